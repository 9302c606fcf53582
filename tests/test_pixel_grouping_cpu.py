"""Host side of the pixel-grouping evaluation model: registry / config surface, no CPU fallback, and the golden fixture tied to the
host metric (evaluation.metrics.proposal_metrics over counts restated by eval_oracle.py)."""
import os

import pytest
import torch

import eval_oracle as O
import pixel_grouping_inputs as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(extra=()):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "partdistillation_amd", "configs", "proposal_generation", "swinl.yaml"),      # a tiny Swin
                     ["MODEL.SWIN.EMBED_DIM", "32", "MODEL.SWIN.DEPTHS", "[2, 2, 2, 2]", "MODEL.SWIN.NUM_HEADS", "[2, 2, 4, 4]",
                      "MODEL.SWIN.WINDOW_SIZE", "4", "MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "PixelGroupingModel"] + list(extra))


def test_registry_and_from_config():
    from partdistillation_amd.compat import META_ARCH_REGISTRY, build_model
    import partdistillation_amd.modeling, partdistillation_amd.pixel_grouping_model  # noqa: F401,E401
    cls = META_ARCH_REGISTRY.get("PixelGroupingModel")
    cfg = _cfg(["PIXEL_GROUPING.NUM_SUPERPIXEL_CLUSTERS", "6", "PIXEL_GROUPING.DISTANCE_METRIC", "dot", "PIXEL_GROUPING.FEATURE_NORMALIZE", "True",
                "PIXEL_GROUPING.BACKBONE_FEATURE_KEY_LIST", "['res3', 'res4']", "PIXEL_GROUPING.DEBUG", "True", "WANDB.VIS_PERIOD_TEST", "7"])
    model = build_model(cfg)
    assert isinstance(model, cls)
    assert (model.num_superpixel_clusters, model.distance_metric, model.feature_normalize, model.debug) == (6, "dot", True, True)
    assert model.backbone_feature_key_list == ["res3", "res4"] and model.wandb_vis_period == 7
    assert model.size_divisibility == cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY
    assert model.pixel_mean.flatten().tolist() == pytest.approx(list(cfg.MODEL.PIXEL_MEAN))
    assert model.pixel_std.flatten().tolist() == pytest.approx(list(cfg.MODEL.PIXEL_STD))
    assert model.num_test_iterations == 0
    # the defaults are the reference's
    d = build_model(_cfg())
    assert (d.num_superpixel_clusters, d.distance_metric, d.feature_normalize, d.backbone_feature_key_list) == (4, "l2", False, ["res4"])


def test_forward_on_cpu_tensors_raises_and_training_mode_asserts():
    from partdistillation_amd.compat import BitMasks, Instances
    from partdistillation_amd.pixel_grouping_model import PixelGroupingModel
    feats, inputs = PG.make_pixel_grouping_inputs()

    class Stub(torch.nn.Module):
        size_divisibility = 32

        def forward(self, x):
            return feats
    model = PixelGroupingModel(backbone=Stub(), size_divisibility=32, pixel_mean=PG.PIXEL_MEAN, pixel_std=PG.PIXEL_STD,
                               backbone_feature_key_list=["res3", "res4"]).eval()
    batched = PG.batched_inputs(inputs, Instances, BitMasks)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(batched)
    model.train()
    with pytest.raises(AssertionError, match="eval only"):
        model(batched)


def test_functions_reject_cpu_tensors():
    from partdistillation_amd.functions import pixel_grouping as G
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.masks_resize([(torch.zeros((1, 8, 8), dtype=torch.bool), (8, 8), (4, 4))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.scores_argmax_resized([(torch.zeros((2, 2, 2)), torch.ones((8, 8), dtype=torch.bool), (8, 8), (8, 8))])


def test_golden_loads_and_its_ar_follows_from_the_host_metric(golden):
    """the reference evaluator's result stored in pixel_grouping.pt == proposal_metrics(counts of the numpy restatement on the stored masks)"""
    from partdistillation_amd.evaluation.metrics import proposal_metrics
    g = golden("pixel_grouping")
    assert set(g) == {tag for tag, _, _ in PG.CONFIGS}
    _, inputs = PG.make_pixel_grouping_inputs()
    for tag, _, _ in PG.CONFIGS:
        imgs = g[tag]["images"]
        assert len(imgs) == len(PG.PIXGROUP["images"]) and g[tag]["near_tie_share"] < 1e-3
        triples = []
        for rec, inp, (_, _, oh, ow, kind) in zip(imgs, inputs, PG.PIXGROUP["images"]):
            pred, gt, obj = O.unpack(rec["pred_masks"]), O.unpack(rec["gt_masks"]), O.unpack(rec["object_mask_resized"])
            assert tuple(pred.shape[1:]) == tuple(gt.shape[1:]) == tuple(obj.shape) == (oh, ow) and gt.shape[0] == inp["part_masks"].shape[0]
            assert pred.shape[0] == {"ellipse": 4, "tiny": 1, "empty": 0}[kind]
            assert torch.equal(pred.any(0), obj) and int(pred.sum()) == int(obj.sum())          # the proposals partition the resized object
            assert rec["centroids"].shape == ((4, 40) if kind == "ellipse" else (1, 40))
            triples.append((pred, torch.ones(pred.shape[0]), gt))
        hits, num_pos = O.recall_counts(triples)
        O.assert_same_dict({"box_proposals": proposal_metrics(hits, num_pos, len(imgs))}, dict(g[tag]["result"]))
