"""fp64 reference of ONE step of the device K-means (include/pd_kmeans.h), plain numpy, no GPU: the slab tables of
functions/kmeans.py, the E-step (scores, first-minimum labels, a derived near-tie flag), the M-step (sums, counts, new
centres, norms, centre moves) and the Lloyd loop with the header's stopping rule; plus the data of the kernel tests
(tests/test_kmeans_kernels_gpu.py), so that tests/test_kmeans_oracle_cpu.py can assert the near-tie share of exactly those
seeds without a GPU.  Pinned against oracle.proposal_generation_ref.kmeans_lloyd_np and scikit-learn in the CPU test."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def make_tables(sizes, slab):
    """blocks [n_blocks, 3] (image, first point, point count) and block_range [B, 2] (first block, number of blocks), int32,
    as kmeans_lloyd_batched builds them: the points of all images concatenated, slabs of `slab` points, none across two images"""
    table, ranges, off = [], [], 0
    for b, n in enumerate(sizes):
        ranges.append((len(table), -(-n // slab)))
        for s0 in range(0, n, slab):
            table.append((b, off + s0, min(slab, n - s0)))
        off += n
    return np.asarray(table, dtype=np.int32).reshape(-1, 3), np.asarray(ranges, dtype=np.int32).reshape(-1, 2)


def img_of_point(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def e_step(X, centers, cnorm, img):
    """X [N, C], centers [B, K, C], cnorm [B, K] (the fp32 values the kernel reads, promoted), img [N] image of every point ->
    scores [N, K] = cnorm[k] - 2 x.c_k (fp64), labels [N] (first minimum), near [N] bool: the gap between the two smallest
    scores is <= tau_n = 4 (C + 2) 2^-24 max_k(sum_i |x_ni| |c_ki| + |cnorm_k|), the worst-case fp32 rounding of two scores
    (a dot product of C terms in any order, the doubling, the subtraction: (C + 2) u each side, twice for the pair)"""
    X, centers, cnorm = np.asarray(X, np.float64), np.asarray(centers, np.float64), np.asarray(cnorm, np.float64)
    N, C = X.shape
    K = centers.shape[1]
    scores, mag = np.empty((N, K)), np.empty((N, K))
    for b in range(centers.shape[0]):
        sel = img == b
        scores[sel] = cnorm[b][None, :] - 2.0 * (X[sel] @ centers[b].T)
        mag[sel] = np.abs(X[sel]) @ np.abs(centers[b]).T + np.abs(cnorm[b])[None, :]
    labels = scores.argmin(1)                                   # numpy: the first minimum
    if K > 1:
        two = np.partition(scores, 1, axis=1)[:, :2]
        near = (two[:, 1] - two[:, 0]) <= 4.0 * (C + 2) * U * mag.max(1)
    else:
        near = np.zeros(N, dtype=bool)
    return scores, labels, near


def m_step(X, labels, centers_old, img, blocks=None):
    """fp64 M-step of every image -> dict: sums [B, K, C], counts [B, K], abs_sums (sum of |x|, for error bounds), centers (an
    empty cluster keeps the old centre), cnorm, shift [B] (total squared move), moves [B, K] (|new_k - old_k|); with `blocks`
    also slab_sums [n_blocks, K, C], slab_abs, slab_counts [n_blocks, K]"""
    X, old = np.asarray(X, np.float64), np.asarray(centers_old, np.float64)
    B, K, C = old.shape
    sums, asum, counts = np.zeros((B, K, C)), np.zeros((B, K, C)), np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            sel = (img == b) & (labels == k)
            sums[b, k], asum[b, k], counts[b, k] = X[sel].sum(0), np.abs(X[sel]).sum(0), sel.sum()
    new = np.where(counts[..., None] > 0, sums / np.maximum(counts, 1)[..., None], old)
    out = dict(sums=sums, abs_sums=asum, counts=counts, centers=new, cnorm=(new * new).sum(-1), shift=((new - old) ** 2).sum((1, 2)),
               moves=np.sqrt(((new - old) ** 2).sum(-1)))
    if blocks is not None:
        nb = len(blocks)
        ss, sa, sc = np.zeros((nb, K, C)), np.zeros((nb, K, C)), np.zeros((nb, K))
        for i, (b, first, npts) in enumerate(blocks):
            x, l = X[first:first + npts], labels[first:first + npts]
            for k in range(K):
                ss[i, k], sa[i, k], sc[i, k] = x[l == k].sum(0), np.abs(x[l == k]).sum(0), (l == k).sum()
        out.update(slab_sums=ss, slab_abs=sa, slab_counts=sc)
    return out


def lloyd(X, init, tol, max_iter=300):
    """one image, the loop of pd_kmeans.h: labels start at -1; an iteration assigns, counts the changed labels, updates, n_iter += 1,
    and is the last one when no label changed or the total squared centre shift <= tol (an absolute number: the caller scales it)
    -> (centres [K, C] fp64, labels of the last E-step, n_iter, strict: stopped because no label changed)"""
    X, centers = np.asarray(X, np.float64), np.asarray(init, np.float64)[None].copy()
    img = np.zeros(len(X), dtype=np.int64)
    labels, n_iter, strict = np.full(len(X), -1), 0, False
    while n_iter < max_iter:
        _, new_labels, _ = e_step(X, centers, (centers * centers).sum(-1), img)
        changed = int((new_labels != labels).sum())
        labels = new_labels
        m = m_step(X, labels, centers, img)
        centers = m["centers"]
        n_iter += 1
        strict = changed == 0
        if strict or m["shift"][0] <= tol:
            break
    return centers[0], labels, n_iter, strict


# ---- the data of the kernel tests --------------------------------------------------------------------------------------------------------------
# name: (points per image, C, K, slab, L2-normalised rows)
CASES = {
    "a": ([70, 1, 64, 9], 4, 2, 32, False),          # a one-point image, a one-point trailing slab, the smallest C
    "b": ([333, 40], 260, 4, 32, False),             # C over one 256-channel piece; image 1 has 2 slabs (tail loops of the reduce)
    "c": ([150, 65], 2048, 8, 64, False),            # KMAX = 8 at the largest C: the dynamic LDS request is just over 64 KiB
    "d": ([97], 1028, 5, 32, False),
    "e": ([300, 57, 9], 256, 8, 32, True),           # part-ranking geometry
    "f": ([45], 64, 1, 17, False),                   # K = 1, a slab size that is no power of two
    "g": ([200], 1536, 3, 32, False),
}


RUN_BLOB_SCALE = {"b": 0.25, "g": 0.4}     # make_run: spread of the blob centres (the points have unit spread)
NEAR_TIE_CAP = 0.02                       # share of the points a real-data label comparison may leave out


def _seed(name, kind):
    return 1000 * (ord(name) - ord("a") + 1) + {"exact": 1, "real": 2}[kind]


def make_case(name, kind):
    """-> dict(sizes, C, K, slab, X [N, C] fp32, centers [B, K, C] fp32, cnorm [B, K] fp32, img [N]).
    real: Gaussian blobs at unit spread around K blob centres per image, initial centres = points of the image (of the batch when
    the image has fewer than K).  exact: the same construction in small integers — X and the centres are whole numbers in [-4, 4], so
    every product, dot product (<= 16 * 2048 < 2^24), score, slab sum and count is exact in fp32 in ANY order."""
    sizes, C, K, slab, l2 = CASES[name]
    rng = np.random.default_rng(_seed(name, kind))
    Xs = []
    for n in sizes:
        if kind == "exact":
            blobs = rng.integers(-3, 4, size=(K, C))
            x = np.clip(blobs[rng.integers(K, size=n)] + rng.integers(-1, 2, size=(n, C)), -4, 4).astype(np.float32)
        else:
            blobs = rng.normal(size=(K, C)).astype(np.float32)
            x = (blobs[rng.integers(K, size=n)] + rng.normal(size=(n, C)).astype(np.float32)).astype(np.float32)
            if l2:
                x /= np.linalg.norm(x, axis=1, keepdims=True)
        Xs.append(x)
    X = np.concatenate(Xs)
    centers = np.stack([(x if len(x) >= K else X)[rng.choice(len(x) if len(x) >= K else len(X), K, replace=False)] for x in Xs]).astype(np.float32)
    cnorm = (centers.astype(np.float64) ** 2).sum(-1).astype(np.float32)       # exact data: whole numbers <= 16 * 2048, exact
    return dict(sizes=sizes, C=C, K=K, slab=slab, X=X, centers=centers, cnorm=cnorm, img=img_of_point(sizes))


def make_run(name):
    """the two batches stepped iteration by iteration (bounded against exhaustive E-step), tol = 0 so that a run ends only when no label
    changes: `b` — one blob more than clusters, blob centres close together (long runs), initial centres = points of the image;
    `g` — every initial centre drawn from ONE blob, so that the centres jump far in the first updates and cshift is large"""
    sizes, C, K, slab, _ = CASES[name]
    rng = np.random.default_rng({"b": 7002, "g": 7010}[name])
    Xs, inits = [], []
    for n in sizes:
        blobs = rng.normal(size=(K + 1, C)).astype(np.float32) * RUN_BLOB_SCALE[name]
        which = rng.integers(K + 1, size=n)
        x = (blobs[which] + rng.normal(size=(n, C)).astype(np.float32)).astype(np.float32)
        pool = np.flatnonzero(which == which[0]) if name == "g" else np.arange(n)
        Xs.append(x), inits.append(x[rng.choice(pool, K, replace=False)])
    X, centers = np.concatenate(Xs), np.stack(inits).astype(np.float32)
    cnorm = (centers.astype(np.float64) ** 2).sum(-1).astype(np.float32)
    return dict(sizes=sizes, C=C, K=K, slab=slab, X=X, centers=centers, cnorm=cnorm, img=img_of_point(sizes))

