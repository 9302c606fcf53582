/*
 * pd_dcrf.h — C-ABI of the dense-CRF mean field that cleans up generated part proposals (csrc/dense_crf.hip).
 *
 * Reference: dense_crf() of continuously_postprocess_dcrf.py:23-51 (= utils/utils.py:50-78): pydensecrf's DenseCRF2D with a unary from labels, a
 * spatial Gaussian and a bilateral Gaussian pairwise term, both NORMALIZE_SYMMETRIC with a Potts compatibility, `t` mean-field steps, arg-max.
 * The mean-field equations, the unary, the normalisation and the parameters are the reference's; the Gaussian filters are evaluated EXACTLY
 * inside a box of 3 sigma instead of approximately on the permutohedral lattice (the truncation is this project's own definition):
 *
 *   lab[i] in [0, L)                      rank of the pixel's label among the values present (the caller compresses; uint8 [H, W])
 *   U[l, i]  = -log(p)                    if l == lab[i],   -log((1 - p) / (L - 1)) otherwise
 *   k1(i, j) = exp(-(dx^2 + dy^2) / (2 sd1^2))                                   where max(|dx|, |dy|) <= R1 = ceil(3 sd1), else 0
 *   k2(i, j) = exp(-(dx^2 + dy^2) / (2 sd2^2) - |I_i - I_j|^2 / (2 sc^2))        where max(|dx|, |dy|) <= R2 = ceil(3 sd2), else 0
 *              (j == i included; pixels outside the image do not exist: no clamping, no mirroring)
 *   n_m(i)   = 1 / sqrt(sum_j k_m(i, j) + 1e-20)
 *   Q_0      = softmax_l(-U)
 *   Q[l, i] <- softmax_l(-U[l, i] + compat1 n_1(i) sum_j k1(i, j) n_1(j) Q[l, j] + compat2 n_2(i) sum_j k2(i, j) n_2(j) Q[l, j])
 *              (synchronous: every sum reads the previous Q)
 *
 * One step is pd_dcrf_spatial_message followed by pd_dcrf_bilateral_update, Q ping-ponging between two buffers of the caller; nothing
 * synchronises with the host and no kernel uses atomics, so a result is bit-reproducible.  All arithmetic is fp32; the bilateral kernel
 * spends one hardware exp per pixel pair (the spatial factor is folded into its exponent).
 *
 * Every pointer is a device pointer and must be non-null; maps are contiguous row-major.  2 <= L <= PD_DCRF_MAX_LABELS, H > 0, W > 0,
 * L * H * W < 2^31, 0 < p < 1, sd1, sd2, sc > 0 and R1, R2 <= PD_DCRF_MAX_RADIUS; anything else returns PD_ERR_INVALID_ARG (pd_msda.h)
 * with pd_last_error() set, and nothing is launched.  `stream` = hipStream_t.
 */
#ifndef PD_DCRF_H
#define PD_DCRF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_DCRF_MAX_LABELS 16
#define PD_DCRF_MAX_RADIUS 96         /* box radius ceil(3 sigma) of either Gaussian */

/*
 * image uint8 [H, W, 3], lab uint8 [H, W]  ->
 *   rgb uint32 [H, W]   the colour packed r | g << 8 | b << 16 (what the bilateral kernel stages)
 *   n1, n2 fp32 [H, W]  the two normalisers (n2 from one pass of the bilateral filter over a field of ones)
 *   q0 fp32 [L, H, W]   softmax_l(-U)
 */
int pd_dcrf_prepare(const uint8_t *image, const uint8_t *lab, int32_t H, int32_t W, int32_t L, double p, double sd1, double sd2, double sc,
                    uint32_t *rgb, float *n1, float *n2, float *q0, void *stream);

/*
 * msg[l, i] = compat1 n_1(i) sum_j k1(i, j) n_1(j) q[l, j], as two 1-D passes (rows into tmp, then columns) with a table of
 * exp(-d^2 / (2 sd1^2)): the box-truncated Gaussian is separable, so this is exact.  q, tmp, msg fp32 [L, H, W]; tmp and msg are overwritten.
 */
int pd_dcrf_spatial_message(const float *q, const float *n1, int32_t H, int32_t W, int32_t L, double sd1, double compat1, float *tmp,
                            float *msg, void *stream);

/*
 * q_next[l, i] = softmax_l(-U[l, i] + msg[l, i] + compat2 n_2(i) sum_j k2(i, j) n_2(j) q[l, j]): the bilateral message and the update in
 * one kernel.  q_next must not alias q.
 */
int pd_dcrf_bilateral_update(const uint32_t *rgb, const uint8_t *lab, const float *n2, const float *q, const float *msg, int32_t H, int32_t W,
                             int32_t L, double p, double sd2, double sc, double compat2, float *q_next, void *stream);

/* out[i] = argmax_l q[l, i], the first maximum; out uint8 [H, W] */
int pd_dcrf_argmax(const float *q, int32_t H, int32_t W, int32_t L, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_DCRF_H */
