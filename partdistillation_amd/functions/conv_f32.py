"""fp32 convolutions of the ResNet backbone on own kernels (include/pd_conv_f32.h): exact-f32 MFMA implicit GEMMs with the frozen-BN
affine, the residual add and the ReLU as the forward's epilogue, the shortcut's gradient as the input gradient's addend, and a filter
gradient without atomics (fixed partition, ordered reduce) — so the fp32 parity leg computes the same bits on every machine and in
every run.  Channels-last tensors only.  No fallback here: the caller (modeling/backbone/resnet.py, behind PD_R50_FP32_OWN) asks
`supported` first and otherwise keeps the library convolution."""
import torch
from torch.autograd import Function

from .. import lib as _lib


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _frozen(conv):
    from ..compat.layers import FrozenBatchNorm2d
    return isinstance(getattr(conv, "norm", None), FrozenBatchNorm2d) and conv.bias is None


def _common(x, conv):
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and conv.weight.dtype == torch.float32
            and x.is_contiguous(memory_format=torch.channels_last) and _frozen(conv)
            and _pair(conv.dilation) == (1, 1) and conv.groups == 1)


def shape_supported(conv):
    """the shape rules of pd_conv_f32_supported, restated on the module (no library needed: the CPU tests ask this)"""
    k, s, p = _pair(conv.kernel_size), _pair(conv.stride), _pair(conv.padding)
    return (k[0] == k[1] and s[0] == s[1] and p[0] == p[1] and k[0] in (1, 3) and s[0] in (1, 2) and p[0] == k[0] // 2
            and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0 and _pair(conv.dilation) == (1, 1) and conv.groups == 1
            and _frozen(conv))


def stem_shape_supported(conv):
    return (_pair(conv.kernel_size) == (7, 7) and _pair(conv.stride) == (2, 2) and _pair(conv.padding) == (3, 3) and conv.in_channels == 3
            and conv.out_channels % 64 == 0 and _pair(conv.dilation) == (1, 1) and conv.groups == 1 and _frozen(conv))


def supported(x, conv):
    return shape_supported(conv) and _common(x, conv) and x.shape[1] == conv.in_channels


def stem_supported(x, conv):
    return stem_shape_supported(conv) and _common(x, conv) and x.shape[1] == 3 and not x.requires_grad


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _nhwc(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def _workspace(L, dev, B, ho, wo, ci, co, k):
    return torch.empty(int(L.pd_conv_f32_wgrad_workspace_floats(B, ho, wo, ci, co, k)), dtype=torch.float32, device=dev)


class ConvBnActF32(Function):
    """y = act(conv(x, w) * scale + bias (+ residual)): x [B, Ci, H, W] and residual channels-last fp32, w [Co, Ci, k, k], scale / bias [Co]
    constants (frozen BatchNorm) or None"""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, residual, relu, stride, padding):
        if not x.is_cuda:
            raise RuntimeError("pd_conv_f32_fwd runs on the GPU only (no CPU fallback in partdistillation_amd)")
        x = _nhwc(x)
        B, ci, H, W = x.shape
        co, k = weight.shape[0], weight.shape[2]
        ho, wo = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
        wk = weight.permute(0, 2, 3, 1).contiguous()                   # [Co,k,k,Ci]: free when the filter is stored channels-last
        residual = _nhwc(residual) if residual is not None else None
        y = torch.empty((B, co, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        _lib.check(_lib.load().pd_conv_f32_fwd(x.data_ptr(), wk.data_ptr(), _ptr(scale), _ptr(bias), _ptr(residual), y.data_ptr(), B, H, W, ci,
                                               ho, wo, co, k, stride, padding, int(relu), _lib.current_stream()))
        ctx.relu, ctx.stride, ctx.padding, ctx.has_res = relu, stride, padding, residual is not None
        ctx.save_for_backward(x, weight, scale, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, scale, y = ctx.saved_tensors
        L = _lib.load()
        B, ci, H, W = x.shape
        co, k = weight.shape[0], weight.shape[2]
        dz = _nhwc(dy)
        if ctx.relu:
            dz = dz * (y > 0)                                           # the gradient behind the ReLU: the residual branch takes it as it is
        dres = dz if ctx.has_res and ctx.needs_input_grad[4] else None
        ho, wo = dz.shape[2], dz.shape[3]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            g = dz * scale.view(1, -1, 1, 1) if scale is not None else dz   # ... and behind the affine
            wt = weight.permute(1, 2, 3, 0).contiguous()                # [Ci,k,k,Co]
            dx = torch.empty_like(x)
            _lib.check(L.pd_conv_f32_dgrad(g.data_ptr(), wt.data_ptr(), None, dx.data_ptr(), B, H, W, ci, ho, wo, co, k, ctx.stride, ctx.padding,
                                           _lib.current_stream()))
        if ctx.needs_input_grad[1]:
            ws = _workspace(L, x.device, B, ho, wo, ci, co, k)
            dwk = torch.empty((co, k, k, ci), dtype=torch.float32, device=x.device)
            _lib.check(L.pd_conv_f32_wgrad(dz.data_ptr(), x.data_ptr(), _ptr(scale), dwk.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, ci, ho, wo,
                                           co, k, ctx.stride, ctx.padding, _lib.current_stream()))
            dw = dwk.permute(0, 3, 1, 2)                                # [Co,Ci,k,k] view with channels-last strides
        return dx, dw, None, None, dres, None, None, None


def conv_bn_act(x, weight, scale=None, bias=None, residual=None, relu=False, stride=1, padding=0):
    return ConvBnActF32.apply(x, weight, scale, bias, residual, relu, stride, padding)


class StemConvF32(Function):
    """y = act(conv7x7s2(x, w) * scale + bias): x [B, 3, H, W] channels-last fp32 (no gradient), w [Co, 3, 7, 7]"""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, relu):
        if not x.is_cuda:
            raise RuntimeError("pd_stem7x7_f32_fwd runs on the GPU only (no CPU fallback in partdistillation_amd)")
        x = _nhwc(x)
        B, _, H, W = x.shape
        co = weight.shape[0]
        ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        wk = weight.permute(0, 2, 3, 1).contiguous()
        y = torch.empty((B, co, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        _lib.check(_lib.load().pd_stem7x7_f32_fwd(x.data_ptr(), wk.data_ptr(), _ptr(scale), _ptr(bias), y.data_ptr(), B, H, W, ho, wo, co, int(relu),
                                                  _lib.current_stream()))
        ctx.relu = relu
        ctx.save_for_backward(x, weight, scale, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, scale, y = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        L = _lib.load()
        B, _, H, W = x.shape
        co = weight.shape[0]
        dz = _nhwc(dy)
        if ctx.relu:
            dz = dz * (y > 0)
        ho, wo = dz.shape[2], dz.shape[3]
        ws = _workspace(L, x.device, B, ho, wo, 3, co, 7)
        dwk = torch.empty((co, 7, 7, 3), dtype=torch.float32, device=x.device)
        _lib.check(L.pd_stem7x7_f32_wgrad(dz.data_ptr(), x.data_ptr(), _ptr(scale), dwk.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, ho, wo, co,
                                          _lib.current_stream()))
        return None, dwk.permute(0, 3, 1, 2), None, None, None


def _affine(conv):
    scale, bias = conv.norm.scale_bias()
    return scale.float().contiguous(), bias.float().contiguous()


def conv_module(x, conv, residual=None, relu=True):
    """a Conv2d with a frozen norm, as modeling/backbone/resnet.py::_conv_bn_act runs it"""
    scale, bias = _affine(conv)
    return conv_bn_act(x, conv.weight, scale, bias, residual, relu, _pair(conv.stride)[0], _pair(conv.padding)[0])


def stem_conv(x, conv, relu=True):
    scale, bias = _affine(conv)
    return StemConvF32.apply(x, conv.weight, scale, bias, relu)
