"""Host side of the part-distillation input pipeline (partdistillation_amd/data/device_mapper.py): the base-stage helper of the GPU tests
(tests/input_chain_oracle.py) against Pillow itself, the draw order with the base stage on and off, `load_annotation` of both mappers on
dicts the product's writers save, and the config surface.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import input_chain_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "partdistillation_amd", "configs")
AUG = ("relative_range", (0.9, 0.9))


# ------------------------------------------------------------------------------------------------ helper against Pillow
def _pillow_base(img, base, square):
    from PIL import Image
    H, W = img.shape[:2]
    scale = min(base / H, base / W)
    bh, bw = int(np.round(H * scale)), int(np.round(W * scale))
    out = np.asarray(Image.fromarray(img).resize((bw, bh), Image.BILINEAR))
    if not square:
        return out
    canvas = np.full((base, base, 3), 128, np.uint8)
    canvas[:bh, :bw] = out
    return canvas


@pytest.mark.parametrize("H,W,base", [(90, 120, 40), (333, 500, 64), (50, 37, 64), (64, 64, 64)])
def test_base_image_ref_is_pillow_exact(H, W, base):
    img = O.random_image(np.random.RandomState(H + W + base), H, W)
    for square in (False, True):
        got = O.base_image_ref(img, base, square)
        assert got.shape == ((base, base, 3) if square else O.base_shape(H, W, base) + (3,)) and max(got.shape[:2]) == base
        assert np.array_equal(got, _pillow_base(img, base, square))


def test_chained_apply_equals_the_same_steps_done_with_pillow():
    """base resize + 128 pad, then flip -> crop -> resize -> crop -> pad, every step written directly with Pillow / numpy.  At least one draw
    flips: the 128 band of the square canvas then lies on the LEFT and bleeds through the bilinear taps."""
    from PIL import Image
    from oracle import input_pipeline_ref as R
    rng = np.random.RandomState(11)
    H, W, base, S = 90, 120, 64, 48
    img = O.random_image(rng, H, W)
    masks = O.part_masks(rng, base, base, 3)
    flips = 0
    for _ in range(6):
        p = R.draw_params(rng, base, base, S, 0.3, 2.0, *AUG)
        flips += p["flip"]
        got_i, got_m, got_p = O.chain_ref(img, masks, base, True, p)
        a, mm = _pillow_base(img, base, True), masks
        if p["flip"]:
            a, mm = a[:, ::-1], mm[:, :, ::-1]
        x0, y0, cw, ch = p["crop1"]
        a, mm = a[y0:y0 + ch, x0:x0 + cw], mm[:, y0:y0 + ch, x0:x0 + cw]
        rh, rw = p["resize"]
        a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((rw, rh), Image.BILINEAR))
        mm = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(m).astype(np.uint8)).resize((rw, rh), Image.NEAREST)) for m in mm]).astype(bool)
        ox, oy = p["crop2"]
        a, mm = a[oy:oy + S, ox:ox + S], mm[:, oy:oy + S, ox:ox + S]
        want = np.full((S, S, 3), 128, np.uint8)
        want[:a.shape[0], :a.shape[1]] = a
        wm = np.zeros((3, S, S), bool)
        wm[:, :mm.shape[1], :mm.shape[2]] = mm
        assert np.array_equal(got_i, want) and np.array_equal(got_m, wm)
        assert got_p.sum() == S * S - a.shape[0] * a.shape[1] and not got_p[:a.shape[0], :a.shape[1]].any()
    assert 0 < flips < 6


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("base,square", [(-1, False), (-1, True), (40, False), (40, True)])
def test_draw_order_with_and_without_the_base_stage(base, square):
    """every attempt: ResizeScale(1, 1)'s uniform(1.0, 1.0) and FixedSizeCrop's uniform(0.0, 1.0) of base_aug, in that order and only
    when the base stage is on, then the augmentations' draws (oracle draw_params)"""
    from oracle import input_pipeline_ref as R
    from partdistillation_amd.data import DeviceProposalMapper
    m = DeviceProposalMapper(64, 0.1, 2.0, *AUG, device="cpu", rng=np.random.RandomState(3), base_size=base, square_base=square)
    r = np.random.RandomState(3)
    plain = np.random.RandomState(3)
    same_as_plain = True
    for _ in range(20):
        O.base_draws(r, base, square)
        got = m.draw(90, 120)
        assert got == R.draw_params(r, 90, 120, 64, 0.1, 2.0, *AUG)
        same_as_plain &= got == R.draw_params(plain, 90, 120, 64, 0.1, 2.0, *AUG)
    assert m.rng.get_state()[2] == r.get_state()[2] and np.array_equal(m.rng.get_state()[1], r.get_state()[1])
    assert same_as_plain == (base <= 0)                                   # the base draws really shift the sequence


def test_base_canvas_sizes():
    from partdistillation_amd.data import DeviceProposalMapper
    for H, W, base in [(90, 120, 64), (120, 90, 64), (64, 64, 64), (20, 30, 300), (333, 500, 48), (375, 500, 640)]:
        for square in (False, True):
            m = DeviceProposalMapper(64, device="cpu", base_size=base, square_base=square)
            size, canvas = m.base_canvas(H, W)
            assert size == O.base_shape(H, W, base) and canvas == ((base, base) if square else size)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.base_image(np.zeros((8, 8, 3), np.uint8))


def test_free_base_canvas_is_the_mappers():
    from partdistillation_amd.data import DeviceProposalMapper
    from partdistillation_amd.functions.input_pipeline import base_canvas, base_image
    for H, W, base in [(90, 120, 64), (120, 90, 64), (64, 64, 64), (20, 30, 300), (333, 500, 48), (375, 500, 640)]:
        for square in (False, True):
            m = DeviceProposalMapper(64, device="cpu", base_size=base, square_base=square)
            assert base_canvas(H, W, base, square) == m.base_canvas(H, W)
    with pytest.raises(RuntimeError, match="GPU only"):
        base_image(np.zeros((8, 8, 3), np.uint8), 64, True, 128, False, "cpu")


def test_resample_tables_travel_as_one_int32_buffer():
    """the six tables of a resample in one vector: views of vw, vw, vw * ksize_x, vh, vh, vh * ksize_y entries, in that order"""
    from partdistillation_amd.functions.input_pipeline import pack_tables, resample_coeffs
    xtab, ytab = resample_coeffs(17, 23, 5, 9), resample_coeffs(11, 7, 2, 4)                  # ksize 3 and 5
    table, cuts = pack_tables(xtab + ytab)
    assert table.dtype == np.int32 and table.ndim == 1 and len(cuts) == 5
    views = torch.tensor_split(torch.from_numpy(table), cuts.tolist())                        # what upload_tables does on the device
    assert [v.numel() for v in views] == [9, 9, 9 * 3, 4, 4, 4 * 5] and all(v.dtype == torch.int32 for v in views)
    for v, t in zip(views, xtab + ytab):
        assert np.array_equal(v.numpy(), np.asarray(t).reshape(-1))
    flipped = tuple(t[::-1] for t in xtab)                                                    # reversed views pack like copies
    assert np.array_equal(pack_tables(flipped + ytab)[0][:9], xtab[0][::-1])


def test_the_square_column_pass_entry_is_retired():
    from partdistillation_amd import lib
    assert lib.load().pd_cmd_fn_index(b"pd_resample_cols_u8") == -1 and "pd_resample_cols_u8" not in lib.SIGNATURES
    assert not hasattr(lib.load(), "pd_resample_cols_u8")


# ------------------------------------------------------------------------------------------------ load_annotation
def _masks(h=12, w=16):
    m = np.zeros((3, h, w), bool)
    m[0, 2:6, 2:6] = True                                                 # 16 px
    m[1, 6:10, 8:16] = True                                               # 32 px
    m[2, 0:2, 0:8] = True                                                 # 16 px
    return m


def _instance(masks, labels, scores):
    return types.SimpleNamespace(pred_masks=torch.from_numpy(masks), pred_classes=torch.tensor(labels), scores=torch.tensor(scores))


def _pd_mapper(**kw):
    from partdistillation_amd.data import DevicePartDistillationMapper
    args = dict(device="cpu", base_size=16, square_base=True, class_code_to_class_id={"n01": 7}, min_area_ratio=-1.0,
                min_object_area_ratio=0.001, min_score=-1.0)
    args.update(kw)
    return DevicePartDistillationMapper(32, **args)


def test_part_distillation_load_annotation_round_trips_both_writers(tmp_path):
    """save_generated_part_labels (part ranking) writes part_ratios AND part_scores, save_part_segmentation (part distillation) only
    part_scores (its ratios go under another key); part_labels a tensor, part_scores a numpy array, part_ratios a tensor"""
    from partdistillation_amd import inference
    from partdistillation_amd.utils import rle
    masks = _masks()
    inp = {"file_name": "img/a.JPEG", "image_id": "a", "class_code": "n01"}
    model = types.SimpleNamespace(root_save_path=str(tmp_path))
    saved = inference.save_generated_part_labels(model, inp, 7, _instance(masks, [5, 2, 3], [0.5, 0.75, 0.25]))
    assert torch.is_tensor(saved["part_labels"]) and isinstance(saved["part_scores"], np.ndarray) and torch.is_tensor(saved["part_ratios"])
    path = (str(tmp_path), "n01", "a")

    d = _pd_mapper().load_annotation(path)
    assert d["file_name"] == "img/a.JPEG" and d["image_id"] == "a" and d["class_code"] == "n01" and d["gt_object_class"] == 7
    assert (d["height"], d["width"]) == (12, 16) and len(d["pseudo_annotations"]) == 3
    cats = [a["category_id"] for a in d["pseudo_annotations"]]
    assert cats == [5, 2, 3] and all(type(c) is int for c in cats)                                    # tensor labels become ints
    for a, m in zip(d["pseudo_annotations"], masks):
        assert np.array_equal(rle.decode(a["segmentation"]), m)

    # part_ratios = [16, 32, 16] / 192: >= keeps the parts AT the bound, the next float above it drops them
    bound = float(saved["part_ratios"][0])
    assert [a["category_id"] for a in _pd_mapper(min_area_ratio=bound).load_annotation(path)["pseudo_annotations"]] == [5, 2, 3]
    above = float(np.nextafter(np.float32(bound), np.float32(1)))
    assert [a["category_id"] for a in _pd_mapper(min_area_ratio=above).load_annotation(path)["pseudo_annotations"]] == [2]
    # part_scores: >= as well
    assert [a["category_id"] for a in _pd_mapper(min_score=0.5).load_annotation(path)["pseudo_annotations"]] == [5, 2]
    assert [a["category_id"] for a in _pd_mapper(min_score=0.5000001).load_annotation(path)["pseudo_annotations"]] == [2]
    assert _pd_mapper(min_score=0.8).load_annotation(path) is None                                    # no part kept
    # object_ratio = 64 / 192: >= keeps the image at the bound
    ratio = saved["object_ratio"]
    assert ratio == 64 / 192 and _pd_mapper(min_object_area_ratio=ratio).load_annotation(path) is not None
    assert _pd_mapper(min_object_area_ratio=np.nextafter(ratio, 1.0)).load_annotation(path) is None

    # the part-distillation writer: no "part_ratios" key, so min_area_ratio filters nothing at load time
    inp2 = dict(inp, image_id="b")
    saved2 = inference.save_part_segmentation(model, inp2, _instance(masks, [1, 0, 4], [0.5, 0.75, 0.25]))
    assert "part_ratios" not in saved2
    d2 = _pd_mapper(min_area_ratio=0.9, min_score=0.5).load_annotation((str(tmp_path), "n01", "b"))
    assert [a["category_id"] for a in d2["pseudo_annotations"]] == [1, 0]
    # neither key (hand-made labels): everything is kept
    bare = {k: v for k, v in saved2.items() if k != "part_scores"}
    torch.save(bare, os.path.join(str(tmp_path), "n01", "c"))
    assert len(_pd_mapper(min_area_ratio=0.9, min_score=0.9).load_annotation((str(tmp_path), "n01", "c"))["pseudo_annotations"]) == 3
    # no parts, and a corrupted file
    torch.save(dict(bare, part_masks=[], part_labels=torch.zeros(0, dtype=torch.int64)), os.path.join(str(tmp_path), "n01", "d"))
    assert _pd_mapper().load_annotation((str(tmp_path), "n01", "d")) is None
    with open(os.path.join(str(tmp_path), "n01", "e"), "wb") as f:
        f.write(open(os.path.join(str(tmp_path), "n01", "a"), "rb").read()[:40])
    assert _pd_mapper().load_annotation((str(tmp_path), "n01", "e")) is None
    assert _pd_mapper()((str(tmp_path), "n01", "e")) is None and _pd_mapper(is_train=False)((str(tmp_path), "n01", "d")) is None


def test_proposal_load_annotation_reads_the_generation_models_dict(tmp_path):
    """the keys of ProposalGenerationModel._result: file_name = the image id, file_path = the image file; object_ratio filters with `>`"""
    from partdistillation_amd.data import DeviceProposalMapper
    from partdistillation_amd.utils import rle
    masks = _masks()
    res = {"file_name": "a", "file_path": "img/a.JPEG", "class_code": "n01", "class_name": "tench", "part_mask": rle.masks_to_coco_json(masks),
           "object_ratio": 64 / 192, "height": 12, "width": 16, "class_index": 7}
    os.makedirs(tmp_path / "n01")
    torch.save(res, str(tmp_path / "n01" / "a"))
    path = (str(tmp_path), "n01", "a")

    def mapper(ratio):
        return DeviceProposalMapper(32, device="cpu", min_object_area_ratio=ratio, class_code_to_class_id={"n01": 7})
    d = mapper(0.001).load_annotation(path)
    assert d["file_name"] == "img/a.JPEG" and d["image_id"] == "a" and d["class_code"] == "n01" and d["gt_object_class"] == 7
    assert (d["height"], d["width"]) == (12, 16) and [a["category_id"] for a in d["pseudo_annotations"]] == [0, 0, 0]
    for a, m in zip(d["pseudo_annotations"], masks):
        assert np.array_equal(rle.decode(a["segmentation"]), m)
    assert mapper(np.nextafter(64 / 192, 0.0)).load_annotation(path) is not None
    assert mapper(64 / 192).load_annotation(path) is None                                             # `>`: AT the bound the image goes
    torch.save(dict(res, part_mask=[]), str(tmp_path / "n01" / "b"))
    assert mapper(0.001).load_annotation((str(tmp_path), "n01", "b")) is None
    torch.save(dict(res, part_mask=None), str(tmp_path / "n01" / "c"))
    assert mapper(0.001).load_annotation((str(tmp_path), "n01", "c")) is None
    (tmp_path / "n01" / "d").write_bytes((tmp_path / "n01" / "a").read_bytes()[:40])
    assert mapper(0.001).load_annotation((str(tmp_path), "n01", "d")) is None
    assert mapper(0.001)((str(tmp_path), "n01", "d")) is None                                         # __call__ with a tuple loads first


# ------------------------------------------------------------------------------------------------ config
def _cfg(name, extra):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(os.path.join(CONFIGS, name), ["MODEL.DEVICE", "cpu"] + list(extra))


def test_part_distillation_from_config_reads_its_keys():
    from partdistillation_amd.data import DevicePartDistillationMapper
    extra = ["CUSTOM_DATASETS.BASE_SIZE", "640", "CUSTOM_DATASETS.AUG_NAME_LIST", "['flip','crop','scale']", "INPUT.IMAGE_SIZE", "512",
             "INPUT.MIN_SCALE", "0.25", "INPUT.MAX_SCALE", "1.5", "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", "(0.8, 0.7)",
             "PART_DISTILLATION.SET_IMAGE_SQUARE", "True", "PART_DISTILLATION.MIN_OBJECT_AREA_RATIO", "0.05",
             "PART_DISTILLATION.MIN_AREA_RATIO", "0.02", "PART_DISTILLATION.MIN_SCORE", "0.3"]
    cfg = _cfg("part_distillation/swinb_mask2former.yaml", extra)
    m = DevicePartDistillationMapper.from_config(cfg, class_code_to_class_id={"n01": 3})
    assert (m.base_size, m.square_base, m.image_size, m.min_scale, m.max_scale) == (640, True, 512, 0.25, 1.5)
    assert (m.crop_type, tuple(m.crop_size), m.flip) == ("relative_range", (0.8, 0.7), True)
    assert (m.min_object_area_ratio, m.min_area_ratio, m.min_score, m.is_train) == (0.05, 0.02, 0.3, True)
    assert m.class_code_to_class_id == {"n01": 3} and m.device.type == "cpu"
    t = DevicePartDistillationMapper.from_config(cfg, is_train=False)
    assert not t.is_train and t.base_size == 640 and t.square_base
    plain = _cfg("part_distillation/swinb_mask2former.yaml", ["CUSTOM_DATASETS.BASE_SIZE", "640", "CUSTOM_DATASETS.AUG_NAME_LIST", "['flip']"])
    m = DevicePartDistillationMapper.from_config(plain)
    assert (m.min_scale, m.max_scale, m.crop_type, m.square_base, m.flip) == (1.0, 1.0, None, False, True)
    for name in ("color", "rotation_90"):
        bad = _cfg("part_distillation/swinb_mask2former.yaml", ["CUSTOM_DATASETS.BASE_SIZE", "640", "CUSTOM_DATASETS.AUG_NAME_LIST", f"['flip','{name}']"])
        with pytest.raises(NotImplementedError):
            DevicePartDistillationMapper.from_config(bad)
    with pytest.raises(ValueError, match="BASE_SIZE"):                     # the reference's mapper always resizes to it
        DevicePartDistillationMapper.from_config(_cfg("part_distillation/swinb_mask2former.yaml", []))


def test_proposal_from_config_base_size_is_the_callers():
    from oracle import input_pipeline_ref as R
    from partdistillation_amd.data import DeviceProposalMapper
    extra = ["CUSTOM_DATASETS.BASE_SIZE", "640", "CUSTOM_DATASETS.AUG_NAME_LIST", "['flip','crop','scale']", "INPUT.IMAGE_SIZE", "64",
             "INPUT.MIN_SCALE", "0.1", "INPUT.MAX_SCALE", "2.0", "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", "(0.9, 0.9)"]
    cfg = _cfg("proposal_learning/r50_mask2former.yaml", extra)
    m = DeviceProposalMapper.from_config(cfg, base_size=cfg.CUSTOM_DATASETS.BASE_SIZE, class_code_to_class_id={"n01": 3})
    assert (m.base_size, m.square_base, m.class_code_to_class_id) == (640, False, {"n01": 3})
    for name in ("color", "rotation_90"):
        with pytest.raises(NotImplementedError):
            DeviceProposalMapper.from_config(_cfg("proposal_learning/r50_mask2former.yaml", ["CUSTOM_DATASETS.AUG_NAME_LIST", f"['{name}']"]))
    # the default (-1) ignores CUSTOM_DATASETS.BASE_SIZE, as the reference's from_config does, and draws what it always drew
    m = DeviceProposalMapper.from_config(cfg)
    assert m.base_size == -1
    m.rng = np.random.RandomState(8)
    r = np.random.RandomState(8)
    for _ in range(20):
        assert m.draw(90, 120) == R.draw_params(r, 90, 120, 64, 0.1, 2.0, *AUG)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_cols_canvas_rejects_bad_arguments_before_any_launch():
    """the argument checks of pd_resample_cols_canvas_u8 come before the launch, so they answer without a device"""
    from partdistillation_amd import lib
    L = lib.load()
    good = dict(tmp_rows=8, tmp_w=9, r0=0, ksize=3, vh=12, vw=9, out_h=12, out_w=9, pad=128, planar=0)
    bad = {"vh > out_h": dict(vh=13), "vw > out_w": dict(out_w=8), "vw > tmp_w": dict(vw=10, out_w=10), "ksize 0": dict(ksize=0),
           "out_h 0": dict(out_h=0, vh=0), "out_w -1": dict(out_w=-1, vw=0), "negative vw": dict(vw=-1), "null pointers": {}}
    for what, change in bad.items():
        a = dict(good, **change)
        rc = L.pd_resample_cols_canvas_u8(None, a["tmp_rows"], a["tmp_w"], a["r0"], None, None, None, a["ksize"], a["vh"], a["vw"], a["out_h"],
                                          a["out_w"], a["pad"], a["planar"], None, None)
        assert rc == -1 and "pd_resample_cols_canvas_u8" in L.pd_last_error().decode(), what
        with pytest.raises(lib.PdHipError, match="null pointer" if what == "null pointers" else "bad sizes"):
            lib.check(rc)
