"""Dense-CRF refinement of a label map on the device (include/pd_dcrf.h, csrc/dense_crf.hip): the reference's dense_crf()
(continuously_postprocess_dcrf.py:23-51) with its Gaussian filters evaluated exactly inside a box of 3 sigma instead of on pydensecrf's
permutohedral lattice.  Everything is enqueued on the current stream; nothing is read back to the host."""
import torch

from .. import lib as _lib

MAX_LABELS = _lib.const("PD_DCRF_MAX_LABELS")


def rank_compress(labels, n_labels):
    """labels integer [H, W] -> uint8 [H, W]: the rank of every value among the values present, which is what the reference works with
    (np.unique(..., return_inverse=True)).  ValueError when n_labels is outside [2, 16] (the reference divides by n_labels - 1) or when
    more than n_labels distinct values are present."""
    L = int(n_labels)
    if L < 2 or L > MAX_LABELS:
        raise ValueError(f"dense_crf: n_labels = {L}, 2 <= n_labels <= {MAX_LABELS} required")
    if labels.dim() != 2 or labels.is_floating_point() or labels.is_complex():
        raise ValueError(f"dense_crf: integer labels [H, W] expected, got {labels.dtype} {tuple(labels.shape)}")
    values, inverse = torch.unique(labels, return_inverse=True)
    if values.numel() > L:
        raise ValueError(f"dense_crf: {values.numel()} distinct label values, n_labels = {L}")
    return inverse.to(torch.uint8).contiguous()


def dense_crf(image, labels, n_labels, p=0.7, t=10, sd1=3, sd2=20, sc=13, compat1=3, compat2=10, return_q=False):
    """image uint8 [H, W, 3] (RGB), labels integer [H, W], both on the GPU -> uint8 [H, W]: argmax_l Q[l] after t mean-field steps
    (first maximum); with return_q also Q fp32 [n_labels, H, W].

    The result is in RANK space, like the reference's: label values are replaced by their rank among the values PRESENT in `labels`, so
    an absent value shifts every larger one down.  t = 0 returns the rank map itself."""
    ranks = rank_compress(labels, n_labels)
    if not (image.is_cuda and labels.is_cuda):
        raise RuntimeError("dense_crf runs on the GPU only (no CPU fallback in partdistillation_amd)")
    H, W = (int(s) for s in labels.shape)
    if image.dtype != torch.uint8 or tuple(image.shape) != (H, W, 3):
        raise ValueError(f"dense_crf: uint8 image [{H}, {W}, 3] expected, got {image.dtype} {tuple(image.shape)}")
    L, t = int(n_labels), int(t)
    if t < 0:
        raise ValueError(f"dense_crf: t = {t}")
    if t == 0 and not return_q:
        return ranks
    lib, dev = _lib.load(), labels.device
    image = image.contiguous()
    with torch.cuda.device(dev):
        st = _lib.current_stream()
        rgb = torch.empty((H, W), dtype=torch.int32, device=dev)
        n1, n2 = (torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2))
        q, q_next, tmp, msg = (torch.empty((L, H, W), dtype=torch.float32, device=dev) for _ in range(4))
        _lib.check(lib.pd_dcrf_prepare(image.data_ptr(), ranks.data_ptr(), H, W, L, p, sd1, sd2, sc, rgb.data_ptr(), n1.data_ptr(),
                                       n2.data_ptr(), q.data_ptr(), st))
        for _ in range(t):
            _lib.check(lib.pd_dcrf_spatial_message(q.data_ptr(), n1.data_ptr(), H, W, L, sd1, compat1, tmp.data_ptr(), msg.data_ptr(), st))
            _lib.check(lib.pd_dcrf_bilateral_update(rgb.data_ptr(), ranks.data_ptr(), n2.data_ptr(), q.data_ptr(), msg.data_ptr(), H, W, L,
                                                    p, sd2, sc, compat2, q_next.data_ptr(), st))
            q, q_next = q_next, q
        if t == 0:
            out = ranks
        else:
            out = torch.empty((H, W), dtype=torch.uint8, device=dev)
            _lib.check(lib.pd_dcrf_argmax(q.data_ptr(), H, W, L, out.data_ptr(), st))
    return (out, q) if return_q else out
