"""SupervisedModel on the GPU: the two kernels of its evaluation branch (include/pd_assign.h) against chained F.interpolate and
torch.bincount, the identity case against pd_mask_assign, one batched launch, the model's evaluation and training branches and
Supervised_mIOU_Evaluator against the real reference's outputs (tests/golden/supervised.pt)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import common as C
import eval_oracle as O
import supervised_inputs as S

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (K, h, w, Hp, Wp, Hi, Wi, H, W)
CASES = {"tiny": (1, 4, 4, 16, 16, 16, 16, 16, 16),
         "crop_up": (7, 8, 12, 32, 48, 27, 41, 61, 90),                  # crop + up-scale, K off the chunk size
         "down": (65, 8, 12, 32, 48, 27, 41, 13, 19),
         "wide_row": (200, 6, 80, 24, 320, 20, 300, 20, 300),            # a row wider than one wave's 256-pixel segment; identity sizes
         "strong_down": (33, 6, 300, 24, 1200, 20, 1160, 9, 40),         # the LDS row mix does not fit: taps read from memory
         # the LDS row mix in several chunks of k (K * columns > 1024) and in tiles past the first (their first column is not 0):
         "lds_chunks": (200, 6, 80, 24, 320, 20, 300, 25, 310),          # 2 tiles, ~70 columns: chunks of 14 k
         "lds_down_tiles": (100, 8, 256, 32, 1024, 32, 1024, 21, 683)}   # down-scaled, 3 tiles, ~98 columns: chunks of 10 k


def _inputs(case, seed, with_object, with_cls, G=3):
    K, h, w, Hp, Wp, Hi, Wi, H, W = case
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn((K, h, w), generator=g) * 2).to(DEV)
    scores = (torch.rand((K,), generator=g) * 0.9 + 0.05).to(DEV)
    obj = None
    if with_object:                                                       # blocks, so that whole 256-pixel segments lie outside
        obj = (F.interpolate(torch.rand((1, 1, 3, 4), generator=g), size=(H, W), mode="nearest")[0, 0] > 0.35).to(DEV)
    coq = torch.randint(0, 8, (K,), generator=g, dtype=torch.int32).to(DEV) if with_cls else None
    gt = (torch.rand((G, H, W), generator=g) < 0.4).to(DEV)
    return logits, scores, obj, coq, gt


def _dense(logits, scores, obj, case):
    """-> (v_k before the object mask, v_k, score * sigmoid(v_k))"""
    K, h, w, Hp, Wp, Hi, Wi, H, W = case
    d = F.interpolate(logits[None], size=(Hp, Wp), mode="bilinear", align_corners=False)[0][:, :Hi, :Wi]
    raw = F.interpolate(d[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    v = raw * obj if obj is not None else raw
    return raw, v, scores[:, None, None] * v.sigmoid()


def _check_maps(arg, objmap, positive, obj, raw, v, p):
    """the tie convention of test_pixel_grouping_gpu._check_labels: arg must equal the dense result wherever the dense top-2 gap exceeds
    1e-5 (fewer than 1 % of the pixels may be left out), obj wherever |max_k v_k| exceeds 1e-5.  positive[k] counts v_k > 0 per k, which
    no output map holds: it must equal the dense count up to the OBJECT pixels whose interpolated logit lies within 1e-5 of zero (the
    zeros the object mask makes are exact and never positive); with K = 1 it is the object map's pixel count, exactly."""
    K = v.shape[0]
    if K > 1:
        top2 = p.topk(2, dim=0)[0]
        clear = (top2[0] - top2[1]) > 1e-5
    else:
        clear = torch.ones_like(arg, dtype=torch.bool)
    assert float((~clear).float().mean()) < 0.01
    assert torch.equal(arg.long()[clear], p.argmax(0)[clear])
    vmax = v.max(0)[0]
    sure = vmax.abs() > 1e-5
    assert torch.equal(objmap.bool()[sure], (vmax > 0)[sure])
    unsure = raw.abs() <= 1e-5
    if obj is not None:
        unsure = unsure & obj.bool()[None]
    slack = unsure.flatten(1).sum(1)
    assert int(slack.max()) <= 2                                          # the check bites: at most a couple of pixels per k are excused
    assert bool(((positive.long() - (v > 0).flatten(1).sum(1)).abs() <= slack).all())
    if K == 1:
        assert int(positive[0]) == int(objmap.sum())


def _check_histogram(key, objmap, gt, n, res):
    """won / area / inter / gt_area == bincounts of the kernel's own maps, exactly"""
    won, area, inter, gt_area = res
    k, ob = key.long().flatten(), objmap.bool().flatten()
    valid = (k >= 0) & (k < n)
    assert torch.equal(won, torch.bincount(k[valid], minlength=n))
    assert torch.equal(area, torch.bincount(k[valid & ob], minlength=n))
    G = 0 if gt is None else gt.shape[0]
    assert tuple(inter.shape) == (n, G) and gt_area.shape[0] == G
    for j in range(G):
        t = gt[j].bool().flatten()
        assert torch.equal(inter[:, j], torch.bincount(k[valid & ob & t], minlength=n))
        assert int(gt_area[j]) == int(t.sum())


@pytest.mark.parametrize("with_object,with_cls", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("name", list(CASES))
def test_mask_assign_resized_against_chained_interpolate(name, with_object, with_cls):
    from partdistillation_amd.functions import mask_assign as A
    case = CASES[name]
    K = case[0]
    logits, scores, obj, coq, gt = _inputs(case, 77, with_object, with_cls)
    (arg, objmap, positive, cls), = A.mask_assign_resized([(logits, scores, obj, coq, case[3:5], case[5:7], case[7:9])])
    _check_maps(arg, objmap, positive, obj, *_dense(logits, scores, obj, case))
    hist = [(arg, objmap, gt, K)]
    if with_cls:
        assert torch.equal(cls.long(), torch.where(objmap.bool(), coq.long()[arg.long()], torch.full_like(arg, -1, dtype=torch.long)))
        hist.append((cls, objmap, gt, 8))
    for (key, om, g_, n), res in zip(hist, A.assign_histogram(hist)):
        _check_histogram(key, om, g_, n, res)


def test_histogram_walks_the_gt_masks_in_passes_and_past_one_workgroup():
    """n * (G + 2) + G above the LDS bins (n = 1024, G = 64: passes of 5 masks), more than 8192 pixels, a pixel count off the 8-pixel step,
    keys outside [0, n)"""
    from partdistillation_amd.functions import mask_assign as A
    g = torch.Generator().manual_seed(5)
    H, W = 131, 97
    key = F.interpolate(torch.randint(-1, 1030, (1, 1, 9, 7), generator=g).float(), size=(H, W), mode="nearest")[0, 0].to(torch.int16).to(DEV)
    obj = (torch.rand((H, W), generator=g) < 0.7).to(DEV)
    gt = (torch.rand((64, H, W), generator=g) < 0.3).to(DEV)
    res, = A.assign_histogram([(key, obj, gt, 1024)])
    _check_histogram(key, obj, gt, 1024, res)


def test_identity_case_is_bit_equal_to_pd_mask_assign():
    from partdistillation_amd import lib as L
    from partdistillation_amd.functions import mask_assign as A
    for case, with_object in (((37, 24, 40, 96, 160, 90, 150, 90, 150), True), (CASES["wide_row"], False), (CASES["tiny"], True)):
        K, h, w, Hp, Wp, Hi, Wi, H, W = case
        logits, scores, obj, _, _ = _inputs(case, 91, with_object, False)
        (arg, objmap, positive, _), = A.mask_assign_resized([(logits, scores, obj, None, (Hp, Wp), (Hi, Wi), (H, W))])
        a2 = torch.empty((H, W), dtype=torch.int16, device=DEV)
        o2 = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        p2 = torch.zeros((K,), dtype=torch.int32, device=DEV)
        o8 = obj.to(torch.uint8).contiguous() if obj is not None else None
        L.check(L.load().pd_mask_assign(logits.data_ptr(), scores.data_ptr(), o8.data_ptr() if o8 is not None else None, a2.data_ptr(), o2.data_ptr(),
                                        p2.data_ptr(), K, h, w, Hp, Wp, H, W, L.current_stream()))
        assert torch.equal(arg, a2) and torch.equal(objmap, o2) and torch.equal(positive, p2)


def test_one_batched_launch_with_an_empty_object_no_gt_and_the_k_limit():
    from partdistillation_amd import lib as L
    from partdistillation_amd.functions import mask_assign as A
    cases = [CASES["crop_up"], CASES["down"], (5, 5, 7, 20, 28, 18, 25, 33, 47)]
    ins = [_inputs(c, 300 + i, True, i == 1) for i, c in enumerate(cases)]
    ins[2] = (ins[2][0], ins[2][1], torch.zeros_like(ins[2][2]), None, ins[2][4])               # an all-zero object mask
    items = [(lg, sc, ob, cq, c[3:5], c[5:7], c[7:9]) for (lg, sc, ob, cq, _), c in zip(ins, cases)]
    maps = A.mask_assign_resized(items)
    for (arg, objmap, positive, cls), (lg, sc, ob, cq, _), c in zip(maps, ins, cases):
        _check_maps(arg, objmap, positive, ob, *_dense(lg, sc, ob, c))
    arg, objmap, positive, _ = maps[2]                                    # v = 0 everywhere: the first largest score, no object, nothing positive
    assert bool((arg == int(ins[2][1].argmax())).all()) and not bool(objmap.any()) and not bool(positive.any())
    hist = [(maps[0][0], maps[0][1], ins[0][4], cases[0][0]), (maps[1][3], maps[1][1], None, 8), (maps[2][0], maps[2][1], ins[2][4], cases[2][0])]
    for (key, om, g_, n), res in zip(hist, A.assign_histogram(hist)):     # G = 0 in the middle
        _check_histogram(key, om, g_, n, res)
    big = (A.MAX_K + 1, 2, 2, 8, 8, 8, 8, 8, 8)
    lg, sc, _, _, _ = _inputs(big, 1, False, False)
    with pytest.raises(L.PdHipError, match="K=257"):                      # refused before anything is launched
        A.mask_assign_resized([items[0], (lg, sc, None, None, (8, 8), (8, 8), (8, 8))])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
def _eval_model(agnostic, unique):
    from partdistillation_amd.supervised_model import SupervisedModel
    kind = "agnostic" if agnostic else "classes"
    model = object.__new__(SupervisedModel)
    torch.nn.Module.__init__(model)
    model.register_buffer("pixel_mean", torch.zeros(3, 1, 1, device=DEV), False)
    model.class_agnostic_learning, model.class_agnostic_inference, model.use_unique_per_pixel_label = agnostic, False, unique
    model.apply_masking_with_object_mask, model.num_classes, model.test_topk_per_image = True, (1 if agnostic else 8), S.SUP["topk"][kind]
    return model, kind


def _prepare(tag):
    """model, inputs and targets on the device (uploads synchronise; the inference itself is what the sync check covers)"""
    from partdistillation_amd.compat import BitMasks, ImageList, Instances
    from partdistillation_amd.supervised_model import SupervisedModel
    model, kind = _eval_model(*S.CONFIGS[tag])
    outputs, inputs = S.make_supervised_inputs()
    outputs = {k: v.to(DEV) for k, v in outputs[kind].items()}
    batched = S.batched_inputs(inputs, Instances, BitMasks, DEV)
    images = ImageList.from_tensors([b["image"] for b in batched], S.SUP["size_div"])
    return model, batched, SupervisedModel.prepare_targets(model, batched, images), images, outputs


def _run_eval(tag):
    from partdistillation_amd.inference_supervised import supervised_inference
    return supervised_inference(*_prepare(tag))


def _by_score(masks, scores, classes):
    order = sorted(range(scores.shape[0]), key=lambda i: (float(scores[i]), int(classes[i])))
    return masks[order], scores[order], classes[order]


@pytest.mark.parametrize("tag", list(S.CONFIGS))
def test_supervised_model_eval_vs_reference_golden(golden, tag):
    """labels and kept-proposal sets identical; masks differ from the reference in at most 2e-3 of the pixels (the allowance of the
    pixel-grouping model test; the generator guarantees that fewer than 1e-3 are near-ties); ground truth exact"""
    res = _run_eval(tag)
    for r, rec in zip(res, golden("supervised")["eval"][tag]["images"]):
        assert r["predictions"] is r["proposals"] and r["gt_instances"] is r["gt_masks"]
        p = r["predictions"]
        m, s, c = _by_score(p.pred_masks.cpu(), p.scores.cpu(), p.pred_classes.cpu())
        wm, ws, wc = _by_score(O.unpack(rec["pred_masks"]), rec["scores"], rec["pred_classes"])
        assert m.dtype == torch.bool and m.shape == wm.shape and torch.equal(c, wc) and torch.allclose(s, ws, rtol=1e-5, atol=1e-7)
        assert float((m != wm).float().mean()) <= 2e-3
        # (stricter, and what the evaluator test's tolerance counts: the PIXELS at which any mask differs)
        assert int((m != wm).any(0).sum()) <= 2e-3 * m.shape[-2] * m.shape[-1]
        assert torch.equal(r["gt_instances"].gt_masks.cpu(), O.unpack(rec["gt_masks"]))
        assert torch.equal(r["gt_instances"].gt_classes.cpu(), rec["gt_classes"])


class _Replay:
    training = False

    def __init__(self, batches):
        self.batches = batches

    def __call__(self, i):
        return self.batches[i]


def _instances(masks, **kw):
    from partdistillation_amd.compat import Instances
    r = Instances(tuple(masks.shape[-2:]))
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@pytest.mark.parametrize("tag", list(S.CONFIGS))
def test_evaluator_vs_reference_evaluator(golden, tag):
    from partdistillation_amd.evaluation import Supervised_mIOU_Evaluator, inference_on_dataset
    g = golden("supervised")
    want = g["evaluator"][tag]["result"]
    names = [f"part{i}" for i in range(8)]
    # (1) on the reference's masks: 1e-12
    outs = []
    for rec in g["eval"][tag]["images"]:
        pm, gm = O.unpack(rec["pred_masks"]).to(DEV), O.unpack(rec["gt_masks"]).to(DEV)
        outs.append({"predictions": _instances(pm, pred_masks=pm, pred_classes=rec["pred_classes"].to(DEV), scores=rec["scores"].to(DEV)),
                     "gt_instances": _instances(gm, gt_masks=gm, gt_classes=rec["gt_classes"].to(DEV))})
    ev = Supervised_mIOU_Evaluator(names, num_classes=8, distributed=True)
    got = inference_on_dataset(_Replay([outs[:2], outs[2:]]), [0, 1], ev)
    assert set(got) == {"mIoU", "mACC", "mIoPred"}
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    assert np.array_equal(ev.confusion()[0], g["evaluator"][tag]["conf"].numpy().astype(np.int64))
    # (2) on the model's own masks.  The plain-threshold settings take the dense torch route, the reference's own operations (the
    # CPU test reproduces its masks exactly; on the GPU a logit within rounding of 0 may flip, which the pixel bound below covers
    # for them too).  Tolerance: test_supervised_model_eval_vs_reference_golden allows masks to differ at no more than
    # d = 2e-3 * H * W pixels of an image, d in all over the set; kept sets, labels and the ground truth are identical, so the classes
    # with predicted or ground-truth pixels are the same.  A differing pixel moves one count of the confusion table from its old
    # predicted class to its new one: with d_c the pixels that touch class c, sum_c d_c <= 2 d, and tp_c and the predicted area q_c
    # move by at most d_c while the ground-truth area a_c is fixed.  Then, with U_c >= a_c the union,
    #   |d IoU_c|    = |tp'/U' - tp/U| <= d_c (U + tp) / (U U') <= 2 d_c / a_c
    #   |d ACC_c|    <= d_c / a_c
    #   |d IoPred_c| = |tp'/q' - tp/q| <= min(1, 2 d_c / (q_c - d_c)) <= min(1, 3 d_c / q_c)     (the chord of a convex function up to 1)
    # The first two are linear in d_c and largest for the smallest area, so their sums over the classes are largest with all 2 d pixels
    # on the smallest class.  The third is a fractional knapsack: spend the 2 d pixels on the classes in ascending q_c, q_c / 3 each.
    # The metrics are those sums divided by the number of classes with any / ground-truth / predicted pixels.  In percent:
    conf = g["evaluator"][tag]["conf"].numpy()
    d = 2e-3 * sum(oh * ow for _, _, oh, ow, _ in S.SUP["images"])
    a = conf[:, :-1].sum(0)
    q = conf[:-1, :].sum(1)
    a_min = a[a > 0].min()
    n_any, n_gt, n_pred = int(((a + q) > 0).sum()), int((a > 0).sum()), int((q > 0).sum())
    budget, worst = 2 * d, 0.0
    for qc in sorted(q[q > 0]):
        x = min(budget, qc / 3)
        worst += 3 * x / qc
        budget -= x
    tol = {"mIoU": 100 * 4 * d / (a_min * n_any), "mACC": 100 * 2 * d / (a_min * n_gt), "mIoPred": 100 * worst / n_pred}
    # (classification, per-pixel-unique: 1.0 / 1.2 / 9.4 points; class-agnostic: 2.1 / 1.0 / 3.2; the plain-threshold classification
    # setting has predicted classes of 75 pixels and up, fewer than the allowance, and its mIoPred bound is weak: 0.9 / 1.2 / 31.7)
    print(tag, "tolerances", tol)
    ev2 = Supervised_mIOU_Evaluator(names, num_classes=8, distributed=False)
    res = _run_eval(tag)
    # The evaluator paints masks in their order and the last one covering a pixel wins.  Plain-threshold masks overlap, and their
    # order is that of topk(sorted=False), which differs between the host (the golden) and the device: the model's proposals are put
    # into the golden's order first (matched by score and class), so that only differing pixels remain.
    for r, rec in zip(res, g["eval"][tag]["images"]):
        p = r["predictions"]
        mine = sorted(range(p.scores.shape[0]), key=lambda i, s=p.scores.cpu(), c=p.pred_classes.cpu(): (float(s[i]), int(c[i])))
        rank = sorted(range(rec["scores"].shape[0]), key=lambda i: (float(rec["scores"][i]), int(rec["pred_classes"][i])))
        order = [0] * len(rank)
        for j, i in enumerate(rank):
            order[i] = mine[j]
        order = torch.tensor(order, device=DEV)
        r["predictions"] = _instances(p.pred_masks, pred_masks=p.pred_masks[order], pred_classes=p.pred_classes[order], scores=p.scores[order])
    got2 = inference_on_dataset(_Replay([res]), [0], ev2)
    print(tag, "own masks", got2, "reference", want)
    for k, v in want.items():
        assert abs(got2[k] - v) <= tol[k], (k, got2[k], v, tol[k])


@pytest.mark.parametrize("name,agnostic,nc", [("agnostic", True, 1), ("classes", False, 8)])
def test_supervised_model_train_branch_vs_reference_golden(golden, name, agnostic, nc):
    """losses of one forward at the tolerance of test_meta_arch_train_branch_vs_reference_golden"""
    import test_product_gpu as TP
    from partdistillation_amd.compat import BitMasks, Instances
    from partdistillation_amd.modeling.meta_arch.mask_former_head import MaskFormerHead
    from partdistillation_amd.supervised_model import SupervisedModel
    fx = golden("supervised")["train"][name]
    cfg = dict(C.META, num_classes=nc)
    head = MaskFormerHead(TP._shape_specs(cfg), num_classes=nc, pixel_decoder=TP.build_pixel_decoder(cfg), transformer_predictor=TP.build_decoder(cfg),
                          transformer_in_feature="multi_scale_pixel_decoder")
    head = TP.load_seeded(head, fx["table"], 111)
    model = SupervisedModel(backbone=TP._StubBackbone(C.stub_backbone_weights(cfg)), sem_seg_head=head, criterion=TP.build_criterion(cfg),
                            num_queries=cfg["queries"], num_classes=nc, size_divisibility=32, pixel_mean=S.PIXEL_MEAN, pixel_std=S.PIXEL_STD,
                            test_topk_per_image=10, dataset_name="none", use_wandb=False, class_agnostic_learning=agnostic).to(DEV).train()
    assert sorted(model.state_dict().keys()) == fx["state_dict_keys"]
    batch = []
    for i in C.make_meta_inputs(cfg):
        parts, obj = Instances((i["height"], i["width"])), Instances((i["height"], i["width"]))
        parts.gt_masks, parts.gt_classes = BitMasks(i["masks"].to(DEV)), i["gt_classes"].to(DEV)
        obj.gt_masks = BitMasks(i["masks"].any(0, keepdim=True).to(DEV))
        batch.append({"image": i["image"].to(DEV), "part_instances": parts, "instances": obj, "height": i["height"], "width": i["width"]})
    for t, want in zip(model.prepare_targets(batch, model.preprocess(batch)), fx["labels"]):
        assert torch.equal(t["labels"].cpu(), want)
    rr = C.ReplayRand(9300)
    model.criterion.rand = rr
    losses = model(batch)
    assert rr.calls == int(fx["rand_calls"]) and set(losses) == set(fx["losses"])
    for k, v in fx["losses"].items():
        torch.testing.assert_close(losses[k].double().cpu().reshape(()), v.reshape(()), rtol=2e-3, atol=1e-4, msg=lambda m: f"{k}: {m}")
    torch.testing.assert_close(sum(losses.values()).double().cpu().reshape(()), fx["total"].reshape(()), rtol=1e-3, atol=1e-4)


def test_fused_inference_and_process_do_not_synchronise(golden):
    """under set_sync_debug_mode("error"): the fused route's only synchronisation is read_counts (one copy of integer counts per batch),
    the evaluator's process() has none"""
    import partdistillation_amd.inference_supervised as IS
    from partdistillation_amd.evaluation import Supervised_mIOU_Evaluator
    _run_eval("classes_unique")                                           # warm-up: allocations, pinned rings
    reads, orig = [], IS.read_counts

    def read(t):
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(1)
            return orig(t)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    ev = Supervised_mIOU_Evaluator([f"part{i}" for i in range(8)], num_classes=8)
    ev.reset()
    ev.process(None, _run_eval("agnostic_unique"))                        # warm-up of the evaluator's table and slot
    prepared = [_prepare(tag) for tag in ("agnostic_unique", "classes_unique")]
    torch.cuda.synchronize()
    IS.read_counts = read
    torch.cuda.set_sync_debug_mode("error")
    try:
        for args in prepared:
            ev.process(None, IS.supervised_inference(*args))
    finally:
        torch.cuda.set_sync_debug_mode("default")
        IS.read_counts = orig
    assert len(reads) == 2
