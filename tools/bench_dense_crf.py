"""Times the dense-CRF refinement (functions/dense_crf.py) per 640 x 640 image with the reference's parameters (t = 10, sd1 = 3, sd2 = 20,
sc = 13), in one process:  python tools/bench_dense_crf.py [--calls 5] [--warmup 2] [--size 640]

Per L in {3, 5, 9} (num_k + 1 labels for 2, 4 and 8 clusters; the three L classes of the bilateral kernel) one JSON line with
  ms_per_image        dense_crf() end to end: prepare, 10 x (spatial message + bilateral update), arg-max
  bilateral_ms        one pd_dcrf_bilateral_update launch;  rest_ms = ms_per_image - t * bilateral_ms
  gpairs_per_s        (2 R2 + 1)^2 * H * W pixel pairs of one bilateral launch per second (the nominal window, borders included)
  valu_share          those pairs x the vector instructions the kernel issues per pair (3 subtractions, 4 multiplies or multiply-adds, 1 addition, 1 exp and
                      one multiply-add per label of the L class) against the fp32 vector peak of the MI355X, 157.3 TFLOP/s = 78.65 T
                      instructions x lanes per second
Device events around `calls` calls after a warm-up.  The reference runs this stage as a CPU job (pydensecrf); it cannot be run here, so no
speed-up is quoted."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from partdistillation_amd import lib as _lib  # noqa: E402
from partdistillation_amd.functions.dense_crf import dense_crf, rank_compress  # noqa: E402

PEAK_LANE_OPS = 157.3e12 / 2


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def make(size, L, g):
    """blocky labels (32 x 32 blocks, 5 % of the pixels flipped) and an image coloured by the block's label plus noise"""
    blocks = torch.randint(0, L, ((size + 31) // 32, (size + 31) // 32), generator=g)
    lab = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:size, :size]
    noisy = torch.where(torch.rand((size, size), generator=g) < 0.05, torch.randint(0, L, (size, size), generator=g), lab)
    base = torch.randint(40, 216, (L, 3), generator=g)
    image = (base[lab] + torch.randint(-25, 26, (size, size, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    return image.cuda(), noisy.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=640)
    args = ap.parse_args()
    g, S = torch.Generator().manual_seed(0), args.size
    p, t, sd1, sd2, sc, compat2 = 0.7, 10, 3.0, 20.0, 13.0, 10.0
    lib = _lib.load()
    for L in (3, 5, 9):
        image, labels = make(S, L, g)
        total = timed(lambda: dense_crf(image, labels, L), args.calls, args.warmup)
        ranks = rank_compress(labels, L)
        rgb = torch.empty((S, S), dtype=torch.int32, device="cuda")
        n1, n2 = torch.empty((S, S), device="cuda"), torch.empty((S, S), device="cuda")
        q, q_next, msg = (torch.zeros((L, S, S), device="cuda") for _ in range(3))
        st = _lib.current_stream()
        _lib.check(lib.pd_dcrf_prepare(image.data_ptr(), ranks.data_ptr(), S, S, L, p, sd1, sd2, sc, rgb.data_ptr(), n1.data_ptr(),
                                       n2.data_ptr(), q.data_ptr(), st))

        def bilateral():
            _lib.check(lib.pd_dcrf_bilateral_update(rgb.data_ptr(), ranks.data_ptr(), n2.data_ptr(), q.data_ptr(), msg.data_ptr(), S, S, L, p,
                                                    sd2, sc, compat2, q_next.data_ptr(), st))
        bil = timed(bilateral, args.calls * t, args.warmup)
        R2 = int(math.ceil(3 * sd2))
        pairs = (2 * R2 + 1) ** 2 * S * S
        lc = 4 if L <= 4 else (8 if L <= 8 else 16)
        rate = pairs / (bil * 1e-3)
        print(json.dumps({"size": S, "L": L, "t": t, "ms_per_image": round(total, 2), "bilateral_ms": round(bil, 3),
                          "rest_ms": round(total - t * bil, 2), "gpairs_per_s": round(rate / 1e9, 1),
                          "valu_share": round(rate * (9 + lc) / PEAK_LANE_OPS, 3)}), flush=True)


if __name__ == "__main__":
    main()
