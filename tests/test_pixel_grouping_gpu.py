"""GPU parity of the pixel-grouping evaluation path: the resized label-map kernel against chained F.interpolate, the boolean mask
resize against `F.interpolate(...) != 0` exactly, PixelGroupingModel against the real reference run (tests/golden/pixel_grouping.pt)
and through inference_on_dataset + ProposalEvaluator against the reference evaluator's result."""
import os

import pytest
import torch
import torch.nn.functional as F

import common as C
import eval_oracle as O
import pixel_grouping_inputs as PG

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (K, h, w, Hp, Wp, Hi, Wi, H, W); the last one is strongly down-scaled: its column span does not fit the kernel's LDS row mix
LABEL_SHAPES = [(4, 16, 16, 128, 128, 128, 128, 128, 128), (4, 16, 16, 128, 128, 112, 120, 96, 110), (7, 5, 9, 40, 72, 33, 70, 50, 101),
                (1, 4, 4, 32, 32, 32, 32, 32, 32)]
EXTRA_SHAPE = (32, 6, 300, 24, 600, 20, 580, 9, 40)


def _label_case(shape, seed):
    K, h, w, Hp, Wp, Hi, Wi, H, W = shape
    scores = C.seeded((K, h, w), seed).to(DEV)
    mask = (C.seeded((H, W), seed + 1) > -0.3).to(DEV)
    return scores, mask, (Hp, Wp), (Hi, Wi)


def _check_labels(shape, item, labels, counts):
    K, h, w, Hp, Wp, Hi, Wi, H, W = shape
    scores, mask = item[0], item[1]
    up = F.interpolate(scores[None], size=(Hp, Wp), mode="bilinear", align_corners=False)[:, :, :Hi, :Wi]
    up = F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0]
    want = torch.where(mask, up.argmax(0) + 1, torch.zeros((), dtype=torch.long, device=DEV))
    assert labels.shape == (H, W) and labels.dtype == torch.uint8
    if K > 1:
        top2 = up.topk(2, dim=0)[0]
        clear = (top2[0] - top2[1]) > 1e-5                       # leave out numerical near-ties
    else:
        clear = torch.ones_like(mask)
        assert (labels[mask] == 1).all()
    near = (~clear).float().mean().item()
    print(f"labels {shape}: near-ties {near:.2e}, mismatches on clear pixels {int((labels.long()[clear] != want[clear]).sum())}")
    assert torch.equal(labels.long()[clear], want[clear]) and near < 0.01
    assert (labels[~mask] == 0).all()
    assert torch.equal(counts[:K + 1].long().cpu(), torch.bincount(labels.flatten().long(), minlength=K + 1).cpu())
    assert not counts[K + 1:].any()


@pytest.mark.parametrize("shape", LABEL_SHAPES + [EXTRA_SHAPE])
def test_scores_argmax_resized_kernel_vs_chained_interpolate(shape):
    from partdistillation_amd.functions import pixel_grouping as G
    item = _label_case(shape, 1)
    labels, counts = G.scores_argmax_resized([item])
    _check_labels(shape, item, labels[0], counts[0])


def test_scores_argmax_resized_one_batched_launch():
    from partdistillation_amd.functions import pixel_grouping as G
    shapes = LABEL_SHAPES + [EXTRA_SHAPE]
    items = [_label_case(s, 10 + 2 * i) for i, s in enumerate(shapes)]
    labels, counts = G.scores_argmax_resized(items)
    assert counts.shape == (len(shapes), 33)
    for s, it, lab, cnt in zip(shapes, items, labels, counts):
        _check_labels(s, it, lab, cnt)


def test_scores_argmax_resized_identity_agrees_with_full_size_kernel():
    from partdistillation_amd import lib
    from partdistillation_amd.functions import pixel_grouping as G
    for shape in (LABEL_SHAPES[0], LABEL_SHAPES[3], (4, 16, 16, 128, 128, 112, 120, 112, 120)):
        K, h, w, Hp, Wp, Hi, Wi, H, W = shape
        scores, mask, pad, crop = item = _label_case(shape, 3)
        got = G.scores_argmax_resized([item])[0][0]
        old = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        lib.check(lib.load().pd_scores_argmax_u8(scores.data_ptr(), mask.to(torch.uint8).data_ptr(), old.data_ptr(), K, h, w, Hp, Wp, H, W,
                                                 lib.current_stream()))
        up = F.interpolate(scores[None], size=(Hp, Wp), mode="bilinear", align_corners=False)[0, :, :H, :W]
        clear = (up.topk(2, dim=0)[0].diff(dim=0)[0].abs() > 1e-5) if K > 1 else torch.ones_like(mask)
        assert torch.equal(got[clear], old[clear]) and (~clear).float().mean() < 0.01


# ----------------------------------------------------------------------------------------------------------------------- mask resize
def _resize_ref(src, crop, out):
    return F.interpolate(src[None, :, :crop[0], :crop[1]].float(), size=out, mode="bilinear", align_corners=False)[0] != 0


def _resize_cases():
    """sizes asserted insensitive to rounding by make_golden_pixel_grouping.py (a): (Hp, Wp, Hi, Wi, H, W)"""
    g = torch.Generator().manual_seed(7)
    cases = []
    for Hp, Wp, Hi, Wi, H, W in [(128, 128, 128, 128, 128, 128), (128, 128, 112, 128, 96, 110), (128, 128, 96, 128, 150, 200),
                                 (128, 128, 128, 128, 100, 90), (128, 128, 112, 96, 112, 96)]:
        dense = (torch.rand((3, Hp, Wp), generator=g) < 0.3)
        single = torch.zeros((6, Hp, Wp), dtype=torch.bool)
        single[0, 0, 0] = single[1, Hi - 1, 5] = single[2, 7, Wi - 1] = single[3, Hi - 1, Wi - 1] = True   # corner, the crop's last row / column
        if Hi < Hp:
            single[4, Hi, 3] = True                                                                          # just outside the crop
        if Wi < Wp:
            single[5, 3, Wi] = True
        cases.append((torch.cat([dense, single]).to(DEV), (Hi, Wi), (H, W)))
    return cases


def test_masks_resize_kernel_exact():
    from partdistillation_amd.functions import pixel_grouping as G
    cases = _resize_cases()
    assert any(src[7].any() for src, _, _ in cases) and any(src[8].any() for src, _, _ in cases)   # a pixel below and one right of a crop
    for src, crop, out in cases:
        (dst, area), = G.masks_resize([(src, crop, out)])
        want = _resize_ref(src, crop, out)
        assert dst.dtype == torch.bool and dst.shape == want.shape
        assert torch.equal(dst, want), (crop, out, int((dst != want).sum()))
        assert torch.equal(area, want.flatten(1).sum(1))
        assert want[:3].any() and want[3:7].flatten(1).any(1).all()
        assert not dst[7:].any()                                            # the pixels outside the crop do not leak in
        assert torch.equal(dst.cpu(), PG.masks_resize_ref(src, crop, out))  # and the host restatement of the rule agrees
        (dst8, _), = G.masks_resize([((src.to(torch.uint8) * 255), crop, out)])   # uint8 input, values other than 1
        assert torch.equal(dst8, want)


def test_masks_resize_follows_the_unfused_index_rule_at_sensitive_sizes():
    """sizes at which `scale * (d + 0.5) - 0.5` rounded step by step (ATen's rule, include/pd_grouping.h) and as one fused multiply-add
    give different taps or a different `l1 == 0` pattern: the kernel must follow the former.  The reference here is the host restatement
    (pixel_grouping_inputs.masks_resize_ref), not a library call whose own contraction is the compiler's choice."""
    from partdistillation_amd.functions import pixel_grouping as G
    g = torch.Generator().manual_seed(11)
    items = []
    for (Hi, H), (Wi, W) in (((122, 854), (195, 711)), ((1885, 1537), (122, 854))):
        for n_in, n_out in ((Hi, H), (Wi, W)):
            a, b = PG.axis_taps(n_in, n_out, False), PG.axis_taps(n_in, n_out, True)
            assert not all((x == y).all() for x, y in zip(a, b)), (n_in, n_out)
        items.append(((torch.rand((2, Hi, Wi), generator=g) < 0.3).to(DEV), (Hi, Wi), (H, W)))
    for (src, crop, out), (dst, area) in zip(items, G.masks_resize(items)):
        want, fused = PG.masks_resize_ref(src, crop, out), PG.masks_resize_ref(src, crop, out, fused=True)
        assert not torch.equal(want, fused)                                 # the input tells the two rules apart
        print(f"resize {crop} -> {out}: pixels that differ from the unfused rule {int((dst.cpu() != want).sum())}, from the fused one "
              f"{int((dst.cpu() != fused).sum())}")
        assert torch.equal(dst.cpu(), want)
        assert torch.equal(area.cpu(), want.flatten(1).sum(1))


def test_masks_resize_batched_launch_and_empty_set():
    from partdistillation_amd.functions import pixel_grouping as G
    cases = _resize_cases()[1:]
    empty = (torch.zeros((0, 64, 64), dtype=torch.bool, device=DEV), (64, 64), (50, 70))
    out = G.masks_resize([cases[0], empty, cases[1], cases[2]])
    assert out[1][0].shape == (0, 50, 70) and out[1][1].numel() == 0
    for (src, crop, size), (dst, area) in zip(cases, [out[0], out[2], out[3]]):
        want = _resize_ref(src, crop, size)
        assert torch.equal(dst, want) and torch.equal(area, want.flatten(1).sum(1))
    assert G.masks_resize([empty])[0][0].shape == (0, 50, 70)               # n = 0 alone: no launch


# ----------------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def gold(golden):
    return golden("pixel_grouping")


def _model(metric, norm, feats):
    from partdistillation_amd.pixel_grouping_model import PixelGroupingModel

    class Stub(torch.nn.Module):
        size_divisibility = 32

        def forward(self, x):
            return {k: v.to(x.device) for k, v in feats.items()}
    m = PixelGroupingModel(backbone=Stub(), size_divisibility=PG.PIXGROUP["size_div"], pixel_mean=PG.PIXEL_MEAN, pixel_std=PG.PIXEL_STD,
                           distance_metric=metric, backbone_feature_key_list=["res3", "res4"], num_superpixel_clusters=PG.PIXGROUP["K"],
                           feature_normalize=norm, debug=True)
    return m.to(DEV).eval()


def _setup(gold, tag, metric, norm):
    from partdistillation_amd.compat import BitMasks, Instances
    g = gold[tag]
    feats, inputs = PG.make_pixel_grouping_inputs()
    model = _model(metric, norm, feats)
    model.init_centroids = lambda i: g["images"][i]["centroids"].to(DEV)
    return g, model, PG.batched_inputs(inputs, Instances, BitMasks), inputs


@pytest.mark.parametrize("tag,metric,norm", PG.CONFIGS)
def test_pixel_grouping_model_vs_reference_golden(gold, tag, metric, norm):
    """whole model (stub backbone) with the reference's final centroids as the K-means start"""
    g, model, batched, inputs = _setup(gold, tag, metric, norm)
    res = model(batched)
    assert len(res) == len(g["images"]) and model.num_test_iterations == 1
    kinds = [i[4] for i in PG.PIXGROUP["images"]]
    for b, (r, want, kind) in enumerate(zip(res, g["images"], kinds)):
        prop, gt = r["proposals"], r["gt_masks"]
        want_pred, want_gt, want_obj = O.unpack(want["pred_masks"]), O.unpack(want["gt_masks"]), O.unpack(want["object_mask_resized"])
        assert prop.pred_masks.is_cuda and prop.pred_masks.dtype == torch.bool and gt.gt_masks.dtype == torch.bool
        assert prop.pred_masks.shape == want_pred.shape, (b, prop.pred_masks.shape, want_pred.shape)
        assert prop.image_size == tuple(want_pred.shape[1:]) == (inputs[b]["height"], inputs[b]["width"])
        mismatch = (prop.pred_masks.cpu() != want_pred).any(0).float().mean().item()
        print(f"{tag} image {b} ({kind}): P = {want_pred.shape[0]}, pixels that differ {mismatch:.2e}")
        assert mismatch < 2e-3, (b, mismatch)                              # fp32 re-association at near-ties only
        assert torch.equal(gt.gt_masks.cpu(), want_gt) and gt.pred_masks is gt.gt_masks
        assert torch.equal(model.debug_last["object_masks"][b].cpu(), want_obj)
        assert prop.scores.shape == (want_pred.shape[0],) and bool((prop.scores == 1).all())
        cen = model.debug_last["centroids"][b]
        if kind == "ellipse":
            torch.testing.assert_close(cen.cpu(), want["centroids"], rtol=1e-3, atol=1e-4)
        else:
            assert cen is None and want["centroids"].shape[0] == 1 and not want["centroids"].any()
        if kind == "tiny":                                                  # K or fewer object pixels at feature resolution: the object mask itself
            assert prop.pred_masks.shape[0] == 1 and torch.equal(prop.pred_masks[0].cpu(), want_obj) and want_obj.any()
        if kind == "empty":
            assert prop.pred_masks.shape[0] == 0


@pytest.mark.parametrize("tag,metric,norm", PG.CONFIGS)
def test_pixel_grouping_end_to_end_ar_equals_reference(gold, tag, metric, norm):
    """inference_on_dataset(PixelGroupingModel, ProposalEvaluator) over the golden set: the reference evaluator's AR on the reference's
    outputs (every reference IoU is >= 0.01 away from a threshold, so the near-tie pixels cannot move a recall)"""
    from partdistillation_amd.evaluation import ProposalEvaluator, inference_on_dataset
    g, model, batched, _ = _setup(gold, tag, metric, norm)
    res = inference_on_dataset(model, [batched[:2], batched[2:]], ProposalEvaluator(distributed=False))
    want = g["result"]["box_proposals"]
    got = res["box_proposals"]
    print(tag, got, want)
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_registry_and_config_on_the_device():
    from partdistillation_amd.compat import META_ARCH_REGISTRY, BitMasks, Instances, build_model
    from partdistillation_amd.config import setup_cfg
    import partdistillation_amd.modeling, partdistillation_amd.pixel_grouping_model  # noqa: F401,E401
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = setup_cfg(os.path.join(root, "partdistillation_amd", "configs", "proposal_generation", "swinl.yaml"),       # a tiny Swin
                    ["MODEL.SWIN.EMBED_DIM", "32", "MODEL.SWIN.DEPTHS", "[2, 2, 2, 2]", "MODEL.SWIN.NUM_HEADS", "[2, 2, 4, 4]",
                     "MODEL.SWIN.WINDOW_SIZE", "4", "MODEL.SWIN.DROP_PATH_RATE", "0.0",
                     "MODEL.META_ARCHITECTURE", "PixelGroupingModel", "PIXEL_GROUPING.NUM_SUPERPIXEL_CLUSTERS", "3",
                     "PIXEL_GROUPING.DISTANCE_METRIC", "dot", "PIXEL_GROUPING.BACKBONE_FEATURE_KEY_LIST", "['res3', 'res4']",
                     "PIXEL_GROUPING.FEATURE_NORMALIZE", "True"])
    cls = META_ARCH_REGISTRY.get("PixelGroupingModel")
    torch.manual_seed(0)
    model = build_model(cfg)
    assert isinstance(model, cls) and model.num_superpixel_clusters == 3 and model.distance_metric == "dot" and model.feature_normalize
    assert model.backbone_feature_key_list == ["res3", "res4"] and model.wandb_vis_period == cfg.WANDB.VIS_PERIOD_TEST
    assert model.size_divisibility == cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY
    _, inputs = PG.make_pixel_grouping_inputs()
    batched = PG.batched_inputs(inputs[1:2], Instances, BitMasks)
    model = model.to(DEV).eval()
    model.kmeans_generator = torch.Generator(device=DEV).manual_seed(0)
    (r,) = model(batched)
    P = r["proposals"].pred_masks.shape[0]
    assert 1 <= P <= 3 and tuple(r["proposals"].pred_masks.shape[1:]) == (96, 110) and r["gt_masks"].gt_masks.shape == (3, 96, 110)
    obj = r["proposals"].pred_masks.any(0)
    assert int(r["proposals"].pred_masks.sum()) == int(obj.sum())            # the proposals partition the object
    model.train()
    with pytest.raises(AssertionError, match="eval only"):
        model(batched)
