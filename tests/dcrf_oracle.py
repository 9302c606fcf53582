"""numpy fp64 restatement of the dense-CRF mean field of include/pd_dcrf.h for the dense-CRF tests: brute force over ALL pixel pairs with
the 3-sigma box mask, O((HW)^2) memory and time, meant for the small shapes of CASES only.  Also the maker of the test inputs."""
import functools
import math

import numpy as np

DEFAULTS = dict(p=0.7, t=10, sd1=3, sd2=20, sc=13, compat1=3, compat2=10)
MARGIN = 2e-3                  # pixels whose top-two margin in the oracle's Q is below this are not compared label for label
MARGIN_SHARE = 0.01            # ... and they are at most this share of the pixels (asserted by tests/test_dense_crf_cpu.py)

# the shapes of tests/test_dense_crf_gpu.py: what each one reaches is said there
CASES = {
    "a": dict(H=20, W=24, L=5, sd1=3, sd2=20, sc=13, seed=11),
    "b": dict(H=37, W=70, L=3, sd1=1, sd2=4, sc=13, seed=12),
    "c": dict(H=28, W=40, L=16, sd1=1, sd2=2, sc=30, seed=13, absent=5),
    "d": dict(H=33, W=17, L=2, sd1=2, sd2=6, sc=5, seed=14),
    "e": dict(H=9, W=130, L=8, sd1=1, sd2=3, sc=13, seed=15),
}


def radius(sd):
    return int(math.ceil(3 * sd))


def rank_map(labels):
    values, inverse = np.unique(np.asarray(labels), return_inverse=True)
    return values, inverse.reshape(np.asarray(labels).shape)


def make_inputs(H, W, L, seed, absent=None):
    """a blocky label map (8 x 8 blocks of one random label, then 5 % of the pixels flipped to a random label) and an image whose colour
    is a per-label base colour plus uniform noise of +-25; the colour follows the label BEFORE the flips, so the mean field has flips to
    undo and Q does not saturate everywhere.  With `absent`, the labels are drawn from the L values of 0 .. L without it."""
    rng = np.random.RandomState(seed)
    values = np.array([v for v in range(L + (absent is not None)) if v != absent], dtype=np.int64)
    blocks = rng.randint(0, L, size=((H + 7) // 8, (W + 7) // 8))
    lab = np.kron(blocks, np.ones((8, 8), dtype=np.int64))[:H, :W]
    flip = rng.rand(H, W) < 0.05
    noisy = np.where(flip, rng.randint(0, L, size=(H, W)), lab)
    base = rng.randint(40, 216, size=(L, 3))
    image = base[lab] + rng.randint(-25, 26, size=(H, W, 3))
    return np.clip(image, 0, 255).astype(np.uint8), values[noisy]


def kernels(image, sd1, sd2, sc):
    """k1, k2 fp64 [HW, HW] with the box truncation; pixels outside the image do not exist"""
    H, W, _ = image.shape
    ys, xs = np.divmod(np.arange(H * W, dtype=np.int32), W)
    dx, dy = np.abs(xs[:, None] - xs[None, :]), np.abs(ys[:, None] - ys[None, :])
    box, d2 = np.maximum(dx, dy), (dx * dx + dy * dy).astype(np.float64)
    del dx, dy
    k1 = np.where(box <= radius(sd1), np.exp(-d2 / (2.0 * sd1 * sd1)), 0.0)
    cd = np.zeros_like(d2)
    flat = image.reshape(-1, 3).astype(np.float64)
    for ch in range(3):
        cd += (flat[:, None, ch] - flat[None, :, ch]) ** 2
    k2 = np.where(box <= radius(sd2), np.exp(-d2 / (2.0 * sd2 * sd2) - cd / (2.0 * sc * sc)), 0.0)
    return k1, k2


def normalisers(k):
    return 1.0 / np.sqrt(k.sum(1) + 1e-20)


def softmax0(x):
    e = np.exp(x - x.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def mean_field(image, labels, n_labels, p=0.7, t=10, sd1=3, sd2=20, sc=13, compat1=3, compat2=10, keep=()):
    """-> (labels uint8 [H, W] in rank space, Q fp64 [L, H, W], {step: Q} for the steps listed in `keep`)"""
    image, L = np.asarray(image), int(n_labels)
    H, W, _ = image.shape
    values, lab = rank_map(labels)
    if L < 2 or len(values) > L:
        raise ValueError((L, len(values)))
    lab = lab.reshape(-1)
    U = np.full((L, H * W), -math.log((1.0 - p) / (L - 1)))
    U[lab, np.arange(H * W)] = -math.log(p)
    Q = softmax0(-U)
    kept = {0: Q.reshape(L, H, W)}
    if t > 0:
        k1, k2 = kernels(image, sd1, sd2, sc)
        n1, n2 = normalisers(k1), normalisers(k2)
        k1 *= n1[:, None] * n1[None, :]
        k2 *= n2[:, None] * n2[None, :]
        for step in range(1, t + 1):
            Q = softmax0(-U + compat1 * (Q @ k1.T) + compat2 * (Q @ k2.T))
            if step in keep:
                kept[step] = Q.reshape(L, H, W)
    Q = Q.reshape(L, H, W)
    out = lab.reshape(H, W).astype(np.uint8) if t == 0 else Q.argmax(0).astype(np.uint8)
    return out, Q, kept


def margins(Q):
    """top-two margin of Q [L, H, W] per pixel"""
    s = np.sort(Q, axis=0)
    return s[-1] - s[-2]


def case_params(name):
    c = CASES[name]
    return dict(DEFAULTS, sd1=c["sd1"], sd2=c["sd2"], sc=c["sc"])


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and fp64 results of one of CASES, computed once per process and shared (treat as read-only):
    {"image", "labels", "L", "params", "ranks", "q": {1: Q after one step, 10: Q after ten}, "labels10"}"""
    c = CASES[name]
    image, labels = make_inputs(c["H"], c["W"], c["L"], c["seed"], c.get("absent"))
    params = case_params(name)
    out, _, kept = mean_field(image, labels, c["L"], keep=(1, 10), **params)
    return {"image": image, "labels": labels, "L": c["L"], "params": params, "ranks": rank_map(labels)[1].astype(np.uint8),
            "q": {1: kept[1], 10: kept[10]}, "labels10": out}
