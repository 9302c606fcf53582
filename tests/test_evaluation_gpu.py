"""Device evaluators (include/pd_eval.h, functions/eval_metrics.py, evaluation/): every kernel bit-exact against numpy
(eval_oracle.py), the evaluators end to end against the REAL reference evaluators (tests/golden/eval.pt), the product's evaluation
branches feeding them, and process() without a host synchronisation."""
import numpy as np
import pytest
import torch

import common as C
import eval_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROPOSAL_CASES = ["random", "ellipses", "exact", "ties", "many", "edge"]
MIOU_CASES = ["basic", "matcher_wide", "one_object"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("eval")


def _ellipses(n, H, W, seed, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = torch.rand((n, 2), generator=g) * torch.tensor([H, W], dtype=torch.float32)
    r = (torch.rand((n, 2), generator=g) * scale + 0.05) * torch.tensor([H, W], dtype=torch.float32)
    return ((ys[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((xs[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2 < 1


# ----------------------------------------------------------------------------------------------------------------------- kernels
def test_pack_bit_planes_and_areas_exact():
    """one launch over sets of different sizes: H*W a multiple of 16 (16-byte loads), odd sizes (guarded bytes), a single pixel,
    a set without masks, uint8 masks with values other than 1"""
    from partdistillation_amd.functions import eval_metrics as E
    sets = [_ellipses(5, 64, 80, 1), _ellipses(3, 37, 45, 2), torch.ones((1, 1, 1), dtype=torch.bool), _ellipses(0, 8, 8, 3),
            (_ellipses(4, 33, 64, 4).to(torch.uint8) * 255), _ellipses(2, 1, 65, 5), _ellipses(7, 128, 96, 6, 0.2)]
    out = E.pack_masks([s.to(DEV) for s in sets])
    for s, (bits, area) in zip(sets, out):
        assert torch.equal(bits.cpu(), torch.from_numpy(O.pack_words(s.bool().numpy()))), tuple(s.shape)
        assert torch.equal(area.cpu(), s.bool().flatten(1).sum(1)), tuple(s.shape)


def test_intersections_exact():
    """P = G = 1; 230 masks of which 200 rows are gathered through a permutation against 64 gts (four column tiles); 7 x 17; one launch"""
    from partdistillation_amd.functions import eval_metrics as E
    cases = [(_ellipses(1, 9, 7, 10), None, _ellipses(1, 9, 7, 11)),
             (_ellipses(230, 40, 52, 12, 0.3), torch.randperm(230, generator=torch.Generator().manual_seed(0))[:200], _ellipses(64, 40, 52, 13)),
             (_ellipses(7, 300, 301, 14), torch.tensor([6, 0, 3]), _ellipses(17, 300, 301, 15))]
    packed = E.pack_masks([m.to(DEV) for a, _, b in cases for m in (a, b)])
    items = [(packed[2 * i][0], None if r is None else r.to(DEV), packed[2 * i + 1][0]) for i, (_, r, _) in enumerate(cases)]
    for (a, r, b), got in zip(cases, E.intersections(items)):
        assert torch.equal(got.cpu(), torch.from_numpy(O.intersections(a.numpy(), None if r is None else r.numpy(), b.numpy())))


@pytest.mark.parametrize("n", [6, 100])
def test_confusion_tables_exact(n):
    """n = 6: histogram in LDS; n = 100: (n + 1)^2 > PD_EVAL_LDS_BINS, global atomics.  Images of different sizes and object classes in
    one launch, overlapping masks (last wins), an image without predictions, pixels left to the background on both sides"""
    from partdistillation_amd.functions import eval_metrics as E
    g = torch.Generator().manual_seed(n)
    imgs = []
    for k, (P, G, H, W) in enumerate([(5, 4, 64, 80), (0, 3, 37, 45), (9, 2, 130, 70), (70, 6, 17, 19)]):
        pm, gm = _ellipses(P, H, W, 100 + k, 0.5), _ellipses(G, H, W, 200 + k, 0.5)
        imgs.append((pm, torch.randint(0, n, (P,), generator=g), gm, torch.randint(0, n, (G,), generator=g), [2, 0, 2, 5][k]))
    conf = torch.zeros((7, n + 1, n + 1), dtype=torch.int64, device=DEV)
    packed = E.pack_masks([m.to(DEV) for pm, _, gm, _, _ in imgs for m in (pm, gm)])
    items = [(packed[2 * i][0], pc.to(DEV), packed[2 * i + 1][0], gc.to(DEV), torch.tensor([s], device=DEV), pm[0].numel() if len(pm) else gm[0].numel())
             for i, (pm, pc, gm, gc, s) in enumerate(imgs)]
    E.confusion_add(items, n, conf)
    assert torch.equal(conf.cpu(), torch.from_numpy(O.confusion(imgs, n, 7)))


@pytest.mark.parametrize("name", PROPOSAL_CASES)
def test_proposal_evaluator_golden(gold, name):
    """hits / num_pos bit-exact against numpy, AR exactly the reference's; once image by image and once as one batch"""
    from partdistillation_amd.compat import Instances
    from partdistillation_amd.evaluation import ProposalEvaluator
    case = gold["proposal"][name]
    imgs = O.proposal_images(case)
    outs = []
    for pm, sc, gm in imgs:
        p, gt = Instances(tuple(pm.shape[1:])), Instances(tuple(gm.shape[1:]))
        p.pred_masks, p.scores = pm.to(DEV), sc.to(DEV)
        gt.gt_masks = gm.to(DEV)
        outs.append({"proposals": p, "gt_masks": gt})
    hits, num_pos = O.recall_counts(imgs)
    for batched in (False, True):
        ev = ProposalEvaluator(distributed=False)
        ev.reset()
        if batched:
            ev.process(None, outs)
        else:
            for o in outs:
                ev.process(None, [o])
        h, npos, n = ev.counts()
        assert torch.equal(h, torch.from_numpy(hits)) and torch.equal(npos, torch.from_numpy(num_pos)) and n == len(imgs)
        O.assert_same_dict(ev.evaluate(), dict(case["result"]))


def _miou_outputs(imgs):
    from partdistillation_amd.compat import Instances
    outs = []
    for pm, pc, gm, gc, obj in imgs:
        p, g = Instances(tuple(pm.shape[1:])), Instances(tuple(gm.shape[1:]))
        p.pred_masks, p.pred_classes = pm.to(DEV), pc.to(DEV)
        g.gt_masks, g.gt_classes = gm.to(DEV), gc.to(DEV)
        outs.append({"predictions": p, "gt_instances": g, "gt_object_label": torch.tensor([obj], device=DEV)})
    return outs


@pytest.mark.parametrize("name", MIOU_CASES)
def test_miou_evaluator_and_matcher_golden(gold, name):
    from partdistillation_amd.evaluation import mIOU_Evaluator, mIOU_Matcher
    case = gold["miou"][name]
    gt_n, pred_n = O.gt_num_classes(case), case["pred_n"]
    imgs = O.miou_images(case)
    outs = _miou_outputs(imgs)
    mm = mIOU_Matcher(case["thing_classes"], gt_n, num_classes=pred_n, distributed=False)
    mm.reset()
    mm.process(None, outs[:2])
    mm.process(None, outs[2:])
    assert np.array_equal(mm.confusion(), O.confusion(imgs, max(gt_n, pred_n), 1000))
    got = mm.evaluate()
    assert all(v.is_cuda and v.dtype == torch.int64 for v in got.values())
    assert {k: v.tolist() for k, v in got.items()} == case["match"]
    if "eval" in case:
        ev = mIOU_Evaluator(case["thing_classes"], gt_n, distributed=False)
        ev.reset()
        ev.process(None, outs)
        assert np.array_equal(ev.confusion(), O.confusion(imgs, gt_n, 1000))
        O.assert_same_dict(ev.evaluate(), case["eval"], rel=1e-12)


def test_evaluators_on_reference_inference_outputs(gold, golden):
    """the reference's own evaluation-branch outputs (infer.pt / infer_pd.pt) through the device evaluators"""
    from partdistillation_amd.compat import Instances
    from partdistillation_amd.evaluation import ProposalEvaluator, mIOU_Evaluator
    infer, infer_pd = golden("infer"), golden("infer_pd")
    for tag in ("unique_1", "unique_0"):
        ev = ProposalEvaluator(distributed=False)
        outs = []
        for r in infer[tag]:
            p, g = Instances(tuple(r["pred_masks"].shape[1:])), Instances(tuple(r["gt_masks"].shape[1:]))
            p.pred_masks, p.scores, g.gt_masks = r["pred_masks"].to(DEV), r["scores"].to(DEV), r["gt_masks"].to(DEV)
            outs.append({"proposals": p, "gt_masks": g})
        ev.process(None, outs)
        O.assert_same_dict(ev.evaluate(), dict(gold["infer"][tag]))
    K = C.INFER_PD_CLASSES
    for tag in ("eval_1", "eval_0"):
        imgs = [(r["pred_masks"], r["pred_classes"], t["gt_masks"], t["gt_classes"], int(r["gt_object_label"].reshape(-1)[0]))
                for r, t in zip(infer_pd[tag], infer["unique_1"])]
        ev = mIOU_Evaluator([f"part{i}" for i in range(K)], K, distributed=False)
        ev.process(None, _miou_outputs(imgs))
        O.assert_same_dict(ev.evaluate(), gold["infer_pd"][tag], rel=1e-12)


def test_process_does_not_synchronize(gold):
    """process() only enqueues work: no synchronising call (torch's sync debug mode raises on one) and no torch.cuda.synchronize"""
    from partdistillation_amd.evaluation import ProposalEvaluator, mIOU_Evaluator
    from partdistillation_amd.compat import Instances
    pcase, mcase = gold["proposal"]["ellipses"], gold["miou"]["basic"]
    pouts = []
    for pm, sc, gm in O.proposal_images(pcase)[:2]:
        p, g = Instances(tuple(pm.shape[1:])), Instances(tuple(gm.shape[1:]))
        p.pred_masks, p.scores, g.gt_masks = pm.to(DEV), sc.to(DEV), gm.to(DEV)
        pouts.append({"proposals": p, "gt_masks": g})
    mouts = _miou_outputs(O.miou_images(mcase)[:2])
    pe, me = ProposalEvaluator(distributed=False), mIOU_Evaluator(mcase["thing_classes"], O.gt_num_classes(mcase), distributed=False)
    pe.process(None, pouts)                                   # first calls: tables, staging rings
    me.process(None, mouts)
    torch.cuda.synchronize()
    calls = []
    orig = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: calls.append(1) or orig(*a, **k)
    torch.cuda.set_sync_debug_mode("error")
    try:
        pe.process(None, pouts)
        me.process(None, mouts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize = orig
    assert not calls
    h, num_pos, n = pe.counts()
    hits1, num_pos1 = O.recall_counts(O.proposal_images(pcase)[:2])
    assert torch.equal(h, torch.from_numpy(2 * hits1)) and torch.equal(num_pos, torch.from_numpy(2 * num_pos1)) and n == 4


# ----------------------------------------------------------------------------------------------------------------------- product
def _infer_batch():
    from partdistillation_amd.compat import BitMasks, ImageList, Instances
    outputs, inputs = C.make_infer_inputs()
    batched = []
    for b, i in enumerate(inputs):
        parts, objs = Instances(tuple(i["image"].shape[-2:])), Instances(tuple(i["image"].shape[-2:]))
        parts.gt_masks, parts.gt_classes = BitMasks(i["part_masks"]), i["part_labels"]
        objs.gt_masks, objs.gt_classes = BitMasks(i["object_mask"]), torch.tensor([3 + b])
        batched.append({"image": i["image"], "part_instances": parts, "instances": objs, "height": i["height"], "width": i["width"]})
    images = ImageList.from_tensors([i["image"].to(DEV) for i in inputs], C.INFER["size_div"])
    return outputs, batched, images


class _Recorder:
    def reset(self):
        self.outputs = []

    def process(self, inputs, outputs):
        self.outputs += outputs

    def evaluate(self):
        return {}


@pytest.mark.parametrize("tag,unique,min_score", [("unique_1", True, -1.0), ("unique_0", False, 0.3)])
def test_proposal_model_eval_branch_to_proposal_evaluator(gold, tag, unique, min_score):
    """ProposalModel's device evaluation branch (inference.py) -> ProposalEvaluator through inference_on_dataset.  The counts equal
    numpy's on the same outputs; AR is the reference evaluator's on the reference's outputs up to one recall flip (the device masks
    may differ from the reference's at interpolation near-ties, tests/test_propgen_gpu.py)"""
    import types
    from partdistillation_amd import inference as I
    from partdistillation_amd.evaluation import DatasetEvaluators, ProposalEvaluator, inference_on_dataset
    outputs, batched, images = _infer_batch()
    outputs = {k: v.to(DEV) for k, v in outputs.items()}
    ns = types.SimpleNamespace(device=torch.device(DEV), test_topk_per_image=C.INFER["topk"], wandb_vis_topk=C.INFER["topk"],
                               use_unique_per_pixel_label=unique, minimum_pseudo_mask_ratio=0.02, minimum_pseudo_mask_score=min_score,
                               apply_masking_with_object_mask=True)

    class Model(torch.nn.Module):
        def forward(self, x):
            return I.inference(ns, x, I.prepare_gt_targets(ns, x, images), images, outputs)
    ev, rec = ProposalEvaluator(distributed=False), _Recorder()
    res = inference_on_dataset(Model(), [batched], DatasetEvaluators([ev, rec]))
    hits, num_pos = O.recall_counts([(o["proposals"].pred_masks.cpu(), o["proposals"].scores.cpu(), o["gt_masks"].gt_masks.cpu())
                                     for o in rec.outputs])
    h, npos, n = ev.counts()
    assert torch.equal(h, torch.from_numpy(hits)) and torch.equal(npos, torch.from_numpy(num_pos)) and n == 2
    want = gold["infer"][tag]["box_proposals"]
    got = res["box_proposals"]
    assert list(got) == list(want) and got["# instances"] == want["# instances"]
    for k in want:
        assert abs(got[k] - want[k]) <= 100.0 / (10 * int(num_pos[0])) + 1e-9, (k, got[k], want[k])


def test_part_distillation_match_then_evaluate_protocol(gold):
    """PartDistillationModel's protocol on the device: mode "match" -> mIOU_Matcher -> update_majority_vote_mapping -> mode "eval" ->
    mIOU_Evaluator, each pass through inference_on_dataset.  The mapping equals the reference's; the tables equal numpy's on the same
    outputs; the metrics are the reference's up to the device masks' near-tie pixels (< 2e-3 of them, tests/test_propgen_gpu.py)"""
    import types
    from partdistillation_amd import inference as I
    from partdistillation_amd.evaluation import DatasetEvaluators, inference_on_dataset, mIOU_Evaluator, mIOU_Matcher
    from partdistillation_amd.evaluation.metrics import miou_metrics
    from partdistillation_amd.part_distillation_model import PartDistillationModel
    outputs, batched, images = _infer_batch()
    K = C.INFER_PD_CLASSES
    outputs = {"pred_masks": outputs["pred_masks"].to(DEV), "pred_logits": (C.seeded((2, C.INFER["Q"], K + 1), 5300) * 2).to(DEV)}
    ns = types.SimpleNamespace(device=torch.device(DEV), test_topk_per_image=C.INFER["topk"] * 2, wandb_vis_topk=C.INFER["topk"] * 2,
                               use_unique_per_pixel_label=True, min_pseudo_mask_ratio=0.02, min_pseudo_mask_score=-1.0,
                               apply_masking_with_object_mask=True, num_part_classes=K, mode="match", fg_score_threshold=0.1,
                               use_oracle_classifier=False, majority_vote_mapping={})

    class Model(torch.nn.Module):
        def forward(self, x):
            return I.pd_inference(ns, x, I.prepare_pd_gt_targets(ns, x, images), images, outputs)
    names = [f"part{i}" for i in range(K)]
    matcher = mIOU_Matcher(names, K, num_classes=K, distributed=False)
    mapping = inference_on_dataset(Model(), [batched], matcher)
    assert {k: v.tolist() for k, v in mapping.items()} == gold["pd_chain"]["mapping"]
    PartDistillationModel.update_majority_vote_mapping(ns, mapping)
    ns.mode = "eval"
    ev, rec = mIOU_Evaluator(names, K, distributed=False), _Recorder()
    inference_on_dataset(Model(), [batched], DatasetEvaluators([ev, rec]))
    res = ev.evaluate()
    imgs = [(o["predictions"].pred_masks.cpu(), o["predictions"].pred_classes.cpu(), o["gt_instances"].gt_masks.cpu(),
             o["gt_instances"].gt_classes.cpu(), int(o["gt_object_label"].reshape(-1)[0])) for o in rec.outputs]
    conf = O.confusion(imgs, K, 1000)
    assert np.array_equal(ev.confusion(), conf)
    O.assert_same_dict(res, miou_metrics(conf, names, K), rel=1e-12)
    want = gold["pd_chain"]["eval"]
    assert list(res) == list(want)
    for k in want:
        assert abs(res[k] - want[k]) <= 0.5, (k, res[k], want[k])
