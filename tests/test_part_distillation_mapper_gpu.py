"""Part-distillation input pipeline on the device: pd_resample_cols_canvas_u8 (include/pd_input.h) alone against numpy, the base stage of
DeviceProposalMapper against the Pillow-exact oracle chain (tests/input_chain_oracle.py), and DevicePartDistillationMapper end to end, train
and test.  Everything is integer arithmetic: every comparison is bit-exact."""
import types

import numpy as np
import pytest
import torch

import input_chain_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the kernel alone
def _cols_ref(tmp, r0, ymin, cnt, kk, vh, vw, out_h, out_w, pad, planar):
    out = np.full((out_h, out_w, 3), pad, np.uint8)
    for y in range(vh):
        acc = np.full((vw, 3), 1 << 21, np.int64)
        for j in range(cnt[y]):
            acc += tmp[ymin[y] + j - r0, :vw].astype(np.int64) * int(kk[y, j])
        out[y, :vw] = np.clip(acc >> 22, 0, 255)
    return out.transpose(2, 0, 1) if planar else out


def _cols_call(tmp, r0, ymin, cnt, kk, vh, vw, out_h, out_w, pad, planar, ksize=None, null_out=False):
    from partdistillation_amd import lib
    assert vh == 0 or (int(ymin[:vh].min()) >= r0 and int((ymin + cnt)[:vh].max()) - r0 <= tmp.shape[0])     # the taps stay inside tmp
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (tmp, ymin, cnt, kk)]
    out = torch.full((3, max(out_h, 1), max(out_w, 1)) if planar else (max(out_h, 1), max(out_w, 1), 3), 7, dtype=torch.uint8, device=DEV)
    lib.check(lib.load().pd_resample_cols_canvas_u8(d[0].data_ptr(), tmp.shape[0], tmp.shape[1], r0, d[1].data_ptr(), d[2].data_ptr(),
                                                    d[3].data_ptr(), kk.shape[1] if ksize is None else ksize, vh, vw, out_h, out_w, pad,
                                                    planar, None if null_out else out.data_ptr(), lib.current_stream()))
    return out.cpu().numpy()


# (source rows, output rows of the resize, first, tmp_w, vw, out_h, out_w, planar)
CASES = {
    "upscale_two_x_blocks_bottom_pad_hwc": (37, 64, 0, 300, 300, 70, 300, 0),
    "downscale_wide_taps_right_pad_planar": (90, 33, 0, 260, 257, 33, 260, 1),
    "identity_no_pad_hwc": (8, 8, 0, 8, 8, 8, 8, 0),
    "identity_no_pad_planar": (8, 8, 0, 8, 8, 8, 8, 1),
    "row_window_r0_both_pads_hwc": (90, 40, 5, 45, 41, 38, 50, 0),
    "upscale_both_pads_planar": (20, 47, 0, 70, 66, 50, 259, 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_cols_canvas_kernel_against_numpy(case):
    from partdistillation_amd.functions.input_pipeline import resample_coeffs
    src_rows, res_rows, first, tmp_w, vw, out_h, out_w, planar = CASES[case]
    vh = min(res_rows - first, out_h)
    ymin, cnt, kk = resample_coeffs(src_rows, res_rows, first, vh)
    r0, r1 = int(ymin.min()), int((ymin + cnt).max())
    if case.startswith("upscale_two"):
        assert kk.shape[1] == 3 and tmp_w > 256 and vh < out_h and vw == out_w
    if case.startswith("downscale"):
        assert kk.shape[1] == 7 and vh == out_h and vw < out_w
    if case.startswith("identity"):
        assert kk.shape[1] == 1 and (vh, vw) == (out_h, out_w)
    if case.startswith("row_window"):
        assert r0 > 0
    rng = np.random.RandomState(len(case))
    tmp = rng.randint(0, 256, (r1 - r0, tmp_w, 3)).astype(np.uint8)
    tmp[rng.rand(*tmp.shape[:2]) < 0.2] = 255                            # saturated runs: the clip and the rounding term at the top
    got = _cols_call(tmp, r0, ymin, cnt, kk, vh, vw, out_h, out_w, 128, planar)
    assert np.array_equal(got, _cols_ref(tmp, r0, ymin, cnt, kk, vh, vw, out_h, out_w, 128, planar))


@pytest.mark.parametrize("planar", [0, 1])
def test_cols_canvas_kernel_all_pad_and_bad_arguments(planar):
    from partdistillation_amd import lib
    from partdistillation_amd.functions.input_pipeline import resample_coeffs
    ymin, cnt, kk = resample_coeffs(8, 12, 0, 12)
    tmp = np.random.RandomState(1).randint(0, 256, (8, 9, 3)).astype(np.uint8)
    got = _cols_call(tmp, 0, ymin, cnt, kk, 0, 9, 12, 300, 77, planar)                                # vh = 0: an all-pad canvas
    assert got.shape == ((3, 12, 300) if planar else (12, 300, 3)) and (got == 77).all()
    got = _cols_call(tmp, 0, ymin, cnt, kk, 12, 0, 12, 9, 5, planar)                                  # vw = 0 likewise
    assert (got == 5).all()
    assert np.array_equal(_cols_call(tmp, 0, ymin, cnt, kk, 12, 9, 12, 9, 128, planar),               # the good call the bad ones vary
                          _cols_ref(tmp, 0, ymin, cnt, kk, 12, 9, 12, 9, 128, planar))
    bad = {"vh > out_h": dict(vh=13), "vw > out_w": dict(out_w=8), "vw > tmp_w": dict(vw=10, out_w=10), "ksize 0": dict(ksize=0),
           "out_h 0": dict(out_h=0, vh=0), "out_w 0": dict(out_w=0, vw=0), "negative vh": dict(vh=-1), "null out": dict(null_out=True)}
    for what, change in bad.items():
        args = dict(vh=12, vw=9, out_h=12, out_w=9, ksize=None, null_out=False)
        args.update(change)
        with pytest.raises(lib.PdHipError, match="pd_resample_cols_canvas_u8"):
            _cols_call(tmp, 0, ymin, cnt, kk, args["vh"], args["vw"], args["out_h"], args["out_w"], 128, planar, args["ksize"], args["null_out"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ base stage
def _proposal_mapper(S, rng, base=-1, square=False, lo=0.1, hi=2.0, crop="relative_range", **kw):
    from partdistillation_amd.data import DeviceProposalMapper
    return DeviceProposalMapper(S, lo, hi, crop, (0.8, 0.8) if crop else None, rng=rng, base_size=base, square_base=square, **kw)


@pytest.mark.parametrize("H,W,base,square", [(90, 120, 64, True), (120, 90, 64, True), (64, 64, 64, True), (20, 30, 300, True),
                                             (333, 500, 48, False)])
def test_base_image_against_the_oracle(H, W, base, square):
    img = O.random_image(np.random.RandomState(H + base), H, W)
    mapper = _proposal_mapper(32, None, base, square)
    want = O.base_image_ref(img, base, square)
    got = mapper.base_image(img)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape == mapper.base_canvas(H, W)[1] + (3,)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(mapper.base_image(torch.from_numpy(img), planar=True).cpu().numpy(), want.transpose(2, 0, 1))


@pytest.mark.parametrize("H,W,base,S,square", [(90, 120, 64, 96, True), (300, 200, 128, 64, False)])
def test_chained_transform_is_bit_exact_against_the_oracle_chain(H, W, base, S, square):
    from oracle import input_pipeline_ref as R
    from partdistillation_amd.utils import rle
    rng = np.random.RandomState(H + S)
    img = O.random_image(rng, H, W)
    mapper = _proposal_mapper(S, rng, base, square, min_area_ratio=0.05)
    ch, cw = mapper.base_canvas(H, W)[1]
    masks = O.part_masks(rng, ch, cw, 4)                                   # the pseudo-labels live at the canvas size
    masks[3] = False
    segs = [rle.encode(m) for m in masks]
    canvas_ref = O.base_image_ref(img, base, square)
    canvas = mapper.base_image(img)
    flips = 0
    for _ in range(8):
        p = mapper.draw(ch, cw)
        flips += p["flip"]
        oi, om, opad = R.apply(canvas_ref, masks, p)
        gi, gm, gpad, area = mapper.transform(canvas, segs, p)
        assert np.array_equal(gi.cpu().numpy(), oi.transpose(2, 0, 1)), p
        assert np.array_equal(gm.cpu().numpy(), om), p
        assert np.array_equal(gpad.cpu().numpy(), opad)
        assert area.cpu().tolist() == om.reshape(4, -1).sum(1).tolist()
        assert mapper.select(gm, area).cpu().tolist() == R.filter_instances(om, 0.05).tolist()
    assert flips >= 1                                                     # flipped, the square canvas's 128 band is on the left, under the taps
    with pytest.raises(AssertionError):                                   # labels at the decoded image's size no longer fit
        mapper.transform(canvas, [rle.encode(np.zeros((H, W), bool))], p)


# ------------------------------------------------------------------------------------------------ the mappers end to end
def _call_ref(img, masks, labels, rng, base, square, S, min_ratio, lo=0.1, hi=2.0, crop=("relative_range", (0.8, 0.8))):
    """the reference's __call__ on the oracle: per attempt the base draws, the augmentation draws, the chain, the filters"""
    from oracle import input_pipeline_ref as R
    canvas = O.base_image_ref(img, base, square) if base > 0 else img
    for attempt in range(100):
        O.base_draws(rng, base, square)
        p = R.draw_params(rng, canvas.shape[0], canvas.shape[1], S, lo, hi, *crop)
        oi, om, opad = R.apply(canvas, masks, p)
        keep = R.filter_instances(om, min_ratio)
        if len(keep):
            return oi.transpose(2, 0, 1), om[keep], opad, labels[keep], attempt
    raise AssertionError("the scene never survives the augmentation")


def _pd_mapper(S, rng, base, square, **kw):
    from partdistillation_amd.data import DevicePartDistillationMapper
    return DevicePartDistillationMapper(S, 0.1, 2.0, "relative_range", (0.8, 0.8), rng=rng, base_size=base, square_base=square,
                                        class_code_to_class_id={"n01": 7}, **kw)


def _assert_output(out, want, S):
    oi, om, opad, labels, _ = want
    assert set(out) >= {"image", "padding_mask", "instances", "height", "width", "file_name", "image_id", "class_code", "gt_object_class"}
    assert "pseudo_annotations" not in out and (out["height"], out["width"]) == (S, S) and out["gt_object_class"] == 7
    inst = out["instances"]
    assert all(t.is_cuda for t in (out["image"], out["padding_mask"], inst.gt_masks.tensor, inst.gt_classes))
    assert inst.image_size == (S, S) and inst.gt_masks.tensor.dtype == torch.bool and inst.gt_classes.dtype == torch.int64
    assert np.array_equal(out["image"].cpu().numpy(), oi) and np.array_equal(out["padding_mask"].cpu().numpy(), opad)
    assert np.array_equal(inst.gt_masks.tensor.cpu().numpy(), om) and inst.gt_classes.cpu().tolist() == labels.tolist()
    assert len(inst) == len(labels) >= 1 and bool(inst.gt_masks.tensor.flatten(1).any(1).all())          # every kept mask is non-empty


@pytest.mark.parametrize("H,W,base,S,square", [(90, 120, 64, 96, True), (120, 90, 48, 64, False)])
def test_part_distillation_mapper_training_call(H, W, base, S, square, tmp_path):
    from PIL import Image
    from partdistillation_amd import inference
    from partdistillation_amd.utils import rle
    rng = np.random.RandomState(H)
    img = O.random_image(rng, H, W)
    ch, cw = _pd_mapper(S, None, base, square).base_canvas(H, W)[1]
    masks = O.part_masks(rng, ch, cw, 4)
    masks[1] = False                                                      # an empty pseudo-label: dropped, with its label
    labels = np.array([5, 2, 7, 3])
    want = _call_ref(img, masks, labels, np.random.RandomState(21), base, square, S, 0.05)
    d = {"file_name": "x.png", "image_id": "x", "class_code": "n01", "gt_object_class": 7, "image": img,
         "pseudo_annotations": [{"segmentation": rle.encode(m), "category_id": int(l)} for m, l in zip(masks, labels)]}
    out = _pd_mapper(S, np.random.RandomState(21), base, square, min_area_ratio=0.05)(d)
    _assert_output(out, want, S)
    assert 1 not in out["instances"].gt_classes.tolist() and "image" in d and len(d["pseudo_annotations"]) == 4      # the input is not modified

    # the same image through the files: the labels the part-ranking stage saves + the image on disk, named by a PATH_ONLY tuple
    Image.fromarray(img).save(str(tmp_path / "x.png"))
    inst = types.SimpleNamespace(pred_masks=torch.from_numpy(masks), pred_classes=torch.from_numpy(labels), scores=torch.ones(4))
    inference.save_generated_part_labels(types.SimpleNamespace(root_save_path=str(tmp_path)),
                                         {"file_name": str(tmp_path / "x.png"), "image_id": "x", "class_code": "n01"}, 7, inst)
    loaded = masks.reshape(4, -1).sum(1) / (ch * cw) >= 0.05               # load_annotation: parts of at least min_area_ratio of the IMAGE
    assert 1 <= loaded.sum() < 4
    want2 = _call_ref(img, masks[loaded], labels[loaded], np.random.RandomState(21), base, square, S, 0.05)
    out2 = _pd_mapper(S, np.random.RandomState(21), base, square, min_area_ratio=0.05, min_object_area_ratio=0.001)((str(tmp_path), "n01", "x"))
    _assert_output(out2, want2, S)
    assert out2["file_name"] == str(tmp_path / "x.png") and out2["image_id"] == "x"


@pytest.mark.parametrize("H,W,base,square", [(90, 120, 64, True), (120, 90, 48, False)])
def test_part_distillation_mapper_test_mode(H, W, base, square):
    from partdistillation_amd.utils import rle
    rng = np.random.RandomState(W)
    img = O.random_image(rng, H, W)
    state = np.random.RandomState(5)
    mapper = _pd_mapper(32, state, base, square, is_train=False)
    ch, cw = mapper.base_canvas(H, W)[1]
    masks = O.part_masks(rng, ch, cw, 4)
    masks[2] = False
    segs = [rle.encode(m) for m in masks]
    d = {"file_name": "x.png", "image_id": "x", "class_code": "n01", "gt_object_class": 7, "image": img,
         "pseudo_annotations": [{"segmentation": s, "category_id": l} for s, l in zip(segs, [4, 0, 6, 1])]}
    before = state.get_state()
    out = mapper(d)
    after = state.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])                              # no draws
    assert np.array_equal(out["image"].cpu().numpy(), O.base_image_ref(img, base, square).transpose(2, 0, 1))
    assert (out["height"], out["width"]) == (ch, cw) == tuple(out["image"].shape[1:]) and out["instances"].image_size == (ch, cw)
    assert out["padding_mask"].shape == (ch, cw) and out["padding_mask"].dtype == torch.bool and not bool(out["padding_mask"].any())
    want = np.stack([rle.decode(s) for i, s in enumerate(segs) if i != 2])
    assert np.array_equal(out["instances"].gt_masks.tensor.cpu().numpy(), want) and out["instances"].gt_classes.tolist() == [4, 0, 1]
    assert out["instances"].gt_masks.tensor.is_cuda and out["gt_object_class"] == 7 and "pseudo_annotations" not in out
    # the area-ratio filter is the training one: a bound between the two smaller shares of the labelled pixels leaves the two larger masks
    share = want.reshape(3, -1).sum(1) / want.sum()
    bound = float(np.sort(share)[:2].mean())
    strict = _pd_mapper(32, state, base, square, is_train=False, min_area_ratio=bound)(d)
    assert strict["instances"].gt_classes.tolist() == [c for c, s in zip([4, 0, 1], share) if s > bound] and len(strict["instances"]) == 2
    # no annotations: zero-length instances, in both modes
    for train in (False, True):
        size = (ch, cw) if not train else (32, 32)
        empty = _pd_mapper(32, state, base, square, is_train=train)(dict(d, pseudo_annotations=[]))
        inst = empty["instances"]
        assert len(inst) == 0 and tuple(inst.gt_masks.tensor.shape) == (0,) + size and inst.gt_classes.numel() == 0
        assert tuple(empty["image"].shape) == (3,) + size and (empty["height"], empty["width"]) == size


def test_proposal_mapper_without_base_size_is_unchanged():
    """regression guard: no base_size -> the transform and the call of before, bit for bit, and the draws of before"""
    from oracle import input_pipeline_ref as R
    from partdistillation_amd.utils import rle
    H, W, S = 90, 120, 64
    rng = np.random.RandomState(H + S)
    img = O.random_image(rng, H, W)
    masks = O.part_masks(rng, H, W, 4)
    masks[3] = False
    segs = [rle.encode(m) for m in masks]
    mapper = _proposal_mapper(S, rng, min_area_ratio=0.05)
    assert mapper.base_size == -1 and not mapper.square_base
    for _ in range(4):
        p = mapper.draw(H, W)
        oi, om, opad = R.apply(img, masks, p)
        gi, gm, gpad, area = mapper.transform(img, segs, p)
        assert np.array_equal(gi.cpu().numpy(), oi.transpose(2, 0, 1)) and np.array_equal(gm.cpu().numpy(), om)
        assert np.array_equal(gpad.cpu().numpy(), opad) and area.cpu().tolist() == om.reshape(4, -1).sum(1).tolist()
    want = _call_ref(img, masks, np.zeros(4, dtype=np.int64), np.random.RandomState(2), -1, False, S, 0.05)
    out = _proposal_mapper(S, np.random.RandomState(2), min_area_ratio=0.05)(
        {"file_name": "x.png", "image_id": "x", "class_code": "n01", "gt_object_class": 7, "image": img,
         "pseudo_annotations": [{"segmentation": s, "category_id": 0} for s in segs]})
    _assert_output(out, want, S)
