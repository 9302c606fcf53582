"""The R50 backbone in fp32 on the own convolutions (modeling/backbone/resnet.py behind OWN_FP32, functions/conv_f32.py) against the
same module in float64 on the CPU, next to the library route on the same GPU; bit-identical repeats; the routes the switch must not
touch; and the fp32 oracle step of test_product_gpu.py::test_full_step_fp32_vs_oracle with the switch on."""
import copy
import os
import sys

import pytest
import torch

import common as C
from oracle import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "partdistillation_amd", "configs", "proposal_learning", "r50_mask2former.yaml")
MODULE = "partdistillation_amd.functions.conv_f32"


def _resnet():
    from partdistillation_amd.modeling.backbone import resnet
    return resnet


def _backbone(seed=0):
    """build_resnet_backbone at the shipped R50 settings with seeded filters and frozen-BN statistics: (fp32 on the GPU, float64 on the CPU)"""
    from partdistillation_amd import lib
    lib.load()
    from partdistillation_amd.compat import ShapeSpec
    from partdistillation_amd.config import setup_cfg
    cfg = setup_cfg(YAML, [])
    net = _resnet().build_resnet_backbone(cfg, ShapeSpec(channels=3))
    net.load_state_dict(C.seeded_weights(C.table_of(net.state_dict()), 31 + seed), strict=False)
    g = torch.Generator().manual_seed(seed + 1)
    for name, m in net.named_modules():                             # non-trivial frozen statistics that keep the activations O(1)
        if type(m).__name__ == "FrozenBatchNorm2d":
            gain = 0.3 if name.endswith("conv3.norm") else 1.4      # (a small residual branch; the others make up for the ReLU's halving)
            var = torch.rand(m.bias.shape, generator=g) * 0.5 + 0.75
            m.weight.copy_(gain * (torch.rand(m.weight.shape, generator=g) * 0.4 + 0.8) * var.sqrt())
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
            m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
            m.running_var.copy_(var)
            m._cache = None
    ref = copy.deepcopy(net).double()
    for m in ref.modules():
        if hasattr(m, "_cache"):
            m._cache = None
    return net.to(DEV), ref


def _input(seed=9):
    return C.seeded((2, 3, 64, 96), seed)


def _run(net, x, gseed=5):
    """forward + backward from seeded output gradients -> (outputs, filter gradients)"""
    for p in net.parameters():
        p.grad = None
    outs = net(x)
    keys = sorted(outs)
    gout = [C.seeded(outs[k].shape, gseed + i).to(outs[k]) for i, k in enumerate(keys)]
    torch.autograd.backward([outs[k] for k in keys], gout)
    return ({k: v.detach().double().cpu() for k, v in outs.items()},
            {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None})


def _count_calls(monkeypatch):
    """how often the own route ran: [convolutions, stems]"""
    from partdistillation_amd.functions import conv_f32
    n = [0, 0]
    body, stem = conv_f32.conv_module, conv_f32.stem_conv

    def conv_module(*a, **k):
        n[0] += 1
        return body(*a, **k)

    def stem_conv(*a, **k):
        n[1] += 1
        return stem(*a, **k)
    monkeypatch.setattr(conv_f32, "conv_module", conv_module)
    monkeypatch.setattr(conv_f32, "stem_conv", stem_conv)
    return n


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def _of_max(a, ref):
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def test_whole_backbone_vs_float64_and_library_route(monkeypatch):
    """every stage output and every filter gradient: d_own (relative L2 deviation of the own route from float64) against d_lib (the
    library route's, same GPU).  Both routes sum the same f32 terms; they differ by order and by ReLU masks flipping on near-zero
    pre-activations, so d_own <= max(4 d_lib, 1e-6) — a wrong tap reads >= 1e-2 — and d_own's maximum deviation stays below 3e-3 of the
    tensor maximum, the bound of test_full_step_fp32_vs_oracle.  Measured (MI355X): d_own 2.9e-7 .. 7.0e-7, d_own / d_lib 1.1 .. 1.6."""
    resnet = _resnet()
    net, ref = _backbone()
    x = _input(12)
    # A ReLU whose float64 pre-activation lies within f32 rounding distance of zero may come out on the other side in ANY f32 run, and on
    # maps of 2 x 4 x 6 pixels one such flip moves a filter gradient by percents of its maximum (seen on the CPU's own fp32 run at other
    # seeds: 5.6e-2 on res4.5.conv3 from one element at -3.8e-7).  That would measure the draw, not the kernels, so the input seed is the
    # one of 9 .. 16 whose reference keeps every pre-activation furthest from zero, and the margin is asserted here: 3e-7 of the tensor
    # maximum, against stage outputs that deviate by < 1e-6 in relative L2 and far less near zero, where few terms are large.
    margin = []
    with monkeypatch.context() as mp:
        relu_ = resnet.F.relu_
        mp.setattr(resnet.F, "relu_", lambda t: (margin.append(float(t.detach().abs().min() / t.detach().abs().max())), relu_(t))[1])
        ro, rg = _run(ref, x.double())
    assert len(margin) == 49 and min(margin) > 3e-7, min(margin)
    monkeypatch.setattr(resnet, "OWN_FP32", False)
    lo, lg = _run(net, x.to(DEV))
    monkeypatch.setattr(resnet, "OWN_FP32", True)
    calls = _count_calls(monkeypatch)
    oo, og = _run(net, x.to(DEV))
    assert calls == [52, 1], calls                                  # 16 blocks x 3 + 4 shortcuts, and the stem
    assert set(oo) == set(ro) == set(lo) and set(og) == set(rg) == set(lg) and len(og) == 53
    bad = []
    print("%-34s %10s %10s %10s" % ("tensor", "d_own", "d_lib", "own/max"))
    for name, own, libv, r in [(k, oo[k], lo[k], ro[k]) for k in sorted(ro)] + [(k, og[k], lg[k], rg[k]) for k in sorted(rg)]:
        d_own, d_lib, m_own = _l2(own, r), _l2(libv, r), _of_max(own, r)
        print("%-34s %10.2e %10.2e %10.2e" % (name, d_own, d_lib, m_own))
        if not (d_own <= max(4 * d_lib, 1e-6) and m_own < 3e-3):
            bad.append((name, d_own, d_lib, m_own))
    assert not bad, bad


def test_forward_and_backward_twice_are_bit_identical(monkeypatch):
    monkeypatch.setattr(_resnet(), "OWN_FP32", True)
    net, _ = _backbone(1)
    x = _input(10).to(DEV)
    o1, g1 = _run(net, x)
    o2, g2 = _run(net, x)
    assert len(g1) == 53
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_switch_off_and_bf16_autocast_are_untouched(monkeypatch):
    """switch off: the new module is not even imported, and importing it changes nothing; bf16 autocast with the switch on: the new
    branch does not fire, the outputs are those of the switch-off run"""
    resnet = _resnet()
    net, _ = _backbone(2)
    x = _input(11).to(DEV)
    monkeypatch.setattr(resnet, "OWN_FP32", False)
    # the library's convolutions are compared with themselves bit for bit: ask it for its deterministic kernels (by default two calls in a
    # row differ in the last bits: measured 2.9e-6 .. 8.0e-6 on the fp32 stage outputs, one bf16 ulp under autocast)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    import partdistillation_amd.functions as pkg
    saved, attr = sys.modules.pop(MODULE, None), pkg.__dict__.pop("conv_f32", None)      # as in a process that never imported it
    try:
        with torch.no_grad():
            net(x)                                                  # the library picks its algorithms on the first call of a shape
            before = net(x)
        assert MODULE not in sys.modules and "conv_f32" not in pkg.__dict__
    finally:
        if saved is not None:
            sys.modules[MODULE] = saved
        if attr is not None:
            pkg.conv_f32 = attr
    from partdistillation_amd.functions import conv_f32  # noqa: F401
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        after = net(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            net(x)
            amp_off = net(x)
        monkeypatch.setattr(resnet, "OWN_FP32", True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp_on = net(x)
    assert calls == [0, 0]
    for k in before:
        print(k, "switch off, before / after the import: max |diff|", float((before[k] - after[k]).abs().max()),
              "; bf16 autocast, switch off / on:", float((amp_on[k].float() - amp_off[k].float()).abs().max()))
    for k in before:
        assert torch.equal(before[k], after[k]), k
        assert amp_on[k].dtype == amp_off[k].dtype and torch.equal(amp_on[k], amp_off[k]), k


# ----------------------------------------------------------------------------- the fp32 oracle step with the switch on
def _toy_cfg(extra=()):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(YAML, ["MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "20", "MODEL.MASK_FORMER.DEC_LAYERS", "4",
                            "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", "2", "MODEL.MASK_FORMER.TRAIN_NUM_POINTS", "256",
                            "SOLVER.AMP.ENABLED", "False"] + list(extra))


def _randomise(model, seed):
    table = {k: v for k, v in C.table_of(model.state_dict()).items() if not k.startswith("criterion.")}
    sd = C.seeded_weights(table, seed)
    model.load_state_dict(sd, strict=False)
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_full_step_fp32_vs_oracle_on_own_convolutions(monkeypatch):
    """test_product_gpu.py::test_full_step_fp32_vs_oracle — same toy config, batch, replayed draws, oracle call and tolerances — with the
    backbone on the own fp32 convolutions.  Measured (MI355X) deviations of the three backbone filter gradients, of the tensor maximum:
    stem.conv1 1.2e-3, res3.1.conv2 5.0e-4, res5.0.shortcut 4.0e-5 (library route: 7.7e-4 on the R50 filters); they did not fall to the
    head's 1e-6 and move by factors with the order of the sums alone — single ReLU decisions on these toy images set them (DESIGN.md
    "R50 in fp32 on own kernels").  The bound is the existing test's and is not tightened."""
    from partdistillation_amd.compat import build_model
    from partdistillation_amd.engine.synthetic import make_batch
    import partdistillation_amd.modeling, partdistillation_amd.proposal_model  # noqa: F401,E401
    monkeypatch.setattr(_resnet(), "OWN_FP32", True)
    calls = _count_calls(monkeypatch)
    cfg = _toy_cfg()
    model = build_model(cfg).train()
    sd = _randomise(model, 77)
    batch = make_batch(2, 128, n_parts=3, seed=5, device=DEV)
    # ragged sizes: crop the second image / masks to 96x128 -> exercises ImageList + mask padding
    batch[1]["image"] = batch[1]["image"][:, :96].contiguous()
    batch[1]["instances"].gt_masks.tensor = batch[1]["instances"].gt_masks.tensor[:, :96].contiguous()
    rr = C.ReplayRand(4242)
    model.criterion.rand = rr
    losses = model(batch)
    assert calls == [52, 1], calls
    total = sum(losses.values())
    total.backward()
    # oracle
    osd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    obatch = [{"image": b["image"].cpu(), "instances": {"gt_masks": b["instances"].gt_masks.tensor.cpu()}} for b in batch]
    rr2 = C.ReplayRand(4242)
    olosses = R.proposal_model_losses(osd, obatch, rr2, dec_layers=4, enc_layers=2, num_points=256)
    assert rr.calls == rr2.calls and set(losses) == set(olosses)
    for k in olosses:
        torch.testing.assert_close(losses[k].float().cpu().reshape(()), olosses[k].detach().reshape(()), rtol=2e-3, atol=2e-4,
                                   msg=lambda m: f"{k}: {m}")
    sum(olosses.values()).backward()
    named = dict(model.named_parameters())
    checked = 0
    for k in ["backbone.stem.conv1.weight", "backbone.res3.1.conv2.weight", "backbone.res5.0.shortcut.weight",
              "sem_seg_head.pixel_decoder.input_proj.0.0.weight", "sem_seg_head.pixel_decoder.layer_1.weight",
              "sem_seg_head.pixel_decoder.transformer.encoder.layers.1.self_attn.sampling_offsets.weight",
              "sem_seg_head.predictor.query_feat.weight", "sem_seg_head.predictor.class_embed.bias",
              "sem_seg_head.predictor.transformer_cross_attention_layers.2.multihead_attn.in_proj_weight"]:
        a, b = named[k].grad.float().cpu(), osd[k].grad
        scale = b.abs().max().clamp_min(1e-12)
        print("full step fp32 (own convolutions) grad dev", k, f"{((a - b).abs().max() / scale).item():.1e}")
        assert ((a - b).abs().max() / scale).item() < 3e-3, k
        checked += 1
    assert checked == 9
