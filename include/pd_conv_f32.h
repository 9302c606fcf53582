/*
 * pd_conv_f32.h — C-ABI of the fp32 NHWC convolutions of the ResNet backbone in libpd_hip.so (csrc/conv_f32.hip).
 *
 * What they replace.  With autocast off (the fp32 parity runs) every convolution of the R50 backbone went to the library's fp32
 * convolution, whose algorithm — and with it the order of the sums — is picked per machine.  These are the same launches as
 * pd_conv.h's (convolution AND frozen-BN affine, residual add and ReLU in one; transposed convolution AND the sum with the gradient
 * arriving over the shortcut), in exact fp32: f32 operands and f32 accumulation on v_mfma_f32_32x32x2_f32, whose result is a
 * k-ordered fmaf chain.  No floating-point atomics anywhere: two launches on the same operands give the same bits.
 *
 * Layouts (device pointers, 16-byte aligned; everything is float; `stream` = hipStream_t):
 *   activations  NHWC  [batch][h][w][channels]                 (torch channels_last storage of an NCHW-shaped tensor)
 *   filter       [co][k][k][ci]                                (torch channels_last storage of the [co][ci][k][k] weight)
 *   filter^T     [ci][k][k][co]                                (same taps, channel roles swapped: pd_conv_f32_dgrad's operand)
 * Supported body convolutions: ci % 64 == 0, co % 64 == 0, k in {1, 3}, stride in {1, 2}, pad == k / 2, groups = dilation = 1 —
 * every body convolution of R50 / R101 / R152.  pd_conv_f32_supported() says so.  The stem: 7 x 7, stride 2, pad 3, ci == 3,
 * co % 64 == 0.  Any batch, hi, wi >= 1; ho = (hi + 2 pad - k) / stride + 1 (checked).  The functions return PD_ERR_INVALID_ARG
 * (pd_msda.h) for anything else and touch no buffer then.  Taps outside the image are predicated loads of zero.
 */
#ifndef PD_CONV_F32_H
#define PD_CONV_F32_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pd_conv_f32_supported(int ci, int co, int k, int stride, int pad);

/* y[b,oy,ox,:] = act( conv(x, w)[b,oy,ox,:] * scale[:] + bias[:] (+ residual[b,oy,ox,:]) ),  act = ReLU when relu != 0.
 * scale, bias: [co], nullable (identity / zero); residual: like y, nullable. */
int pd_conv_f32_fwd(const float *x, const float *w, const float *scale, const float *bias, const float *residual, float *y, int batch,
                    int hi, int wi, int ci, int ho, int wo, int co, int k, int stride, int pad, int relu, void *stream);

/* dx[b,iy,ix,:] = sum over taps and co of dz[b,(iy+pad-dy)/stride,(ix+pad-dx)/stride,:] . wt[:,dy,dx,:]  (+ addend[b,iy,ix,:]) — the
 * gradient of pd_conv_f32_fwd's convolution with respect to x, given dz = the gradient at the convolution's output.  wt = the
 * [ci][k][k][co] transpose of the filter; addend: like dx, nullable; dx may alias addend.  Every input pixel is written: one that no
 * tap reaches (1 x 1, stride 2) gets its addend, or zero. */
int pd_conv_f32_dgrad(const float *dz, const float *wt, const float *addend, float *dx, int batch, int hi, int wi, int ci, int ho,
                      int wo, int co, int k, int stride, int pad, void *stream);

/* dw[co][dy][dx][ci] = scale[co] * sum over b, oy, ox of dz[b,oy,ox,co] * x[b, oy*stride + dy - pad, ox*stride + dx - pad, ci]
 * (scale nullable): the gradient of the convolution with respect to its filter, in the filter's own layout.  The pixel sum is cut
 * into S <= 64 equal parts that depend on the sizes only; each part's sums go to workspace[part][co][k][k][ci] and a second kernel
 * adds the parts in ascending order and multiplies by scale.  workspace: at least pd_conv_f32_wgrad_workspace_floats(...) floats
 * (= S * co * k * k * ci), reusable by the next call on the same stream.  The same function sizes the stem's workspace (ci = 3, k = 7). */
int64_t pd_conv_f32_wgrad_workspace_floats(int batch, int ho, int wo, int ci, int co, int k);
int pd_conv_f32_wgrad(const float *dz, const float *x, const float *scale, float *dw, float *workspace, int64_t workspace_floats,
                      int batch, int hi, int wi, int ci, int ho, int wo, int co, int k, int stride, int pad, void *stream);

/* The 7 x 7 / 2 stem (pad 3, ci = 3): x [batch][hi][wi][3], w and dw [co][7][7][3].  The image needs no gradient. */
int pd_stem7x7_f32_fwd(const float *x, const float *w, const float *scale, const float *bias, float *y, int batch, int hi, int wi,
                       int ho, int wo, int co, int relu, void *stream);
int pd_stem7x7_f32_wgrad(const float *dz, const float *x, const float *scale, float *dw, float *workspace, int64_t workspace_floats,
                         int batch, int hi, int wi, int ho, int wo, int co, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_CONV_F32_H */
