"""include/pd_conv_f32.h and functions/conv_f32.py without a GPU: the header parses into the binding, its seven functions are exported, the
predicates say yes to every convolution of the ResNets as build_resnet_backbone makes them and no to what the kernels do not cover, the
switch is off by default and the autograd Functions refuse CPU tensors."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "partdistillation_amd", "configs", "proposal_learning", "r50_mask2former.yaml")
SYMBOLS = ["pd_conv_f32_supported", "pd_conv_f32_fwd", "pd_conv_f32_dgrad", "pd_conv_f32_wgrad_workspace_floats", "pd_conv_f32_wgrad",
           "pd_stem7x7_f32_fwd", "pd_stem7x7_f32_wgrad"]


def test_header_parses_and_declares_the_seven_functions():
    from partdistillation_amd import lib
    sigs, structs, _ = lib.read_headers(lib.INCLUDE)
    for s in SYMBOLS:
        assert s in sigs and s in lib.SIGNATURES, s
    assert sorted(n for n in sigs if "_f32" in n and n.startswith(("pd_conv_f32", "pd_stem7x7_f32"))) == sorted(SYMBOLS)
    P, I, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert sigs["pd_conv_f32_supported"] == (I, [I] * 5)
    assert sigs["pd_conv_f32_fwd"] == (I, [P] * 6 + [I] * 11 + [P])
    assert sigs["pd_conv_f32_dgrad"] == (I, [P] * 4 + [I] * 10 + [P])
    assert sigs["pd_conv_f32_wgrad_workspace_floats"] == (Q, [I] * 6)
    assert sigs["pd_conv_f32_wgrad"] == (I, [P] * 5 + [Q] + [I] * 10 + [P])
    assert sigs["pd_stem7x7_f32_fwd"] == (I, [P] * 5 + [I] * 7 + [P])
    assert sigs["pd_stem7x7_f32_wgrad"] == (I, [P] * 5 + [Q] + [I] * 6 + [P])


def test_the_seven_functions_are_exported():
    from partdistillation_amd import lib
    so = lib.load()
    for s in SYMBOLS:
        assert getattr(so, s) is not None


def _backbone(extra):
    from partdistillation_amd.compat import ShapeSpec
    from partdistillation_amd.config import setup_cfg
    from partdistillation_amd.modeling.backbone.resnet import build_resnet_backbone
    return build_resnet_backbone(setup_cfg(YAML, list(extra)), ShapeSpec(channels=3))


def _convs(net):
    return [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.Conv2d)]


@pytest.mark.parametrize("depth,count", [(50, 53), (101, 104)])
def test_supported_covers_every_convolution_of_the_resnets(depth, count):
    from partdistillation_amd import lib
    from partdistillation_amd.functions import conv_f32
    so = lib.load()
    convs = _convs(_backbone(["MODEL.RESNETS.DEPTH", str(depth)]))
    assert len(convs) == count
    for name, m in convs:
        if name == "stem.conv1":
            assert conv_f32.stem_shape_supported(m) and not conv_f32.shape_supported(m)
            continue
        assert conv_f32.shape_supported(m), name
        assert so.pd_conv_f32_supported(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0]) == 1, name
        assert so.pd_conv_f32_wgrad_workspace_floats(2, 8, 8, m.in_channels, m.out_channels, m.kernel_size[0]) > 0, name
    # CPU tensors are never routed to the kernels
    assert not conv_f32.supported(torch.zeros(1, 64, 4, 4).contiguous(memory_format=torch.channels_last), dict(convs)["res2.0.conv1"])
    assert not conv_f32.stem_supported(torch.zeros(1, 3, 8, 8).contiguous(memory_format=torch.channels_last), dict(convs)["stem.conv1"])


def test_supported_says_no_to_dilation_groups_and_trainable_norms():
    from partdistillation_amd import lib
    from partdistillation_amd.functions import conv_f32
    so = lib.load()
    dil = dict(_convs(_backbone(["MODEL.RESNETS.RES5_DILATION", "2"])))
    assert not conv_f32.shape_supported(dil["res5.0.conv2"]) and not conv_f32.shape_supported(dil["res5.2.conv2"])
    assert conv_f32.shape_supported(dil["res5.0.conv1"]) and conv_f32.shape_supported(dil["res4.0.conv2"])
    m = dil["res5.0.conv2"]
    assert so.pd_conv_f32_supported(m.in_channels, m.out_channels, 3, m.stride[0], m.padding[0]) == 0          # pad 2 != k / 2
    grp = dict(_convs(_backbone(["MODEL.RESNETS.NUM_GROUPS", "2"])))
    assert not any(conv_f32.shape_supported(m) for n, m in grp.items() if n.endswith("conv2"))
    for norm in ("BN", "GN"):
        net = dict(_convs(_backbone(["MODEL.RESNETS.NORM", norm])))
        assert not any(conv_f32.shape_supported(m) for m in net.values())
        assert not conv_f32.stem_shape_supported(net["stem.conv1"])
    for ci, co, k, s, p in [(32, 64, 3, 1, 1), (64, 96, 3, 1, 1), (64, 64, 5, 1, 2), (64, 64, 3, 3, 1), (64, 64, 3, 1, 0), (64, 64, 1, 1, 1),
                            (3, 64, 7, 2, 3), (0, 64, 1, 1, 0)]:
        assert so.pd_conv_f32_supported(ci, co, k, s, p) == 0
    assert so.pd_conv_f32_wgrad_workspace_floats(2, 8, 8, 32, 64, 3) == 0


def test_the_switch_is_off_by_default():
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "PD_R50_FP32_OWN"}
    code = ("import sys; from partdistillation_amd.modeling.backbone import resnet; "
            "assert resnet.OWN_FP32 is False; assert 'partdistillation_amd.functions.conv_f32' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True)


def test_functions_refuse_cpu_tensors():
    from partdistillation_amd.functions import conv_f32
    x = torch.zeros(1, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        conv_f32.conv_bn_act(x, torch.zeros(64, 64, 1, 1), None, None, None, True, 1, 0)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        conv_f32.StemConvF32.apply(torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 7, 7), None, None, True)
