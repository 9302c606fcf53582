"""Every entry point of the device K-means (include/pd_kmeans.h, csrc/kmeans.hip) called directly and compared, call by call, with the
fp64 step reference tests/kmeans_oracle.py.

Two kinds of data.  EXACT: X and the centres are whole numbers in [-4, 4]; every product, dot product, score, slab sum and count is then
exact in fp32 in any order, so labels, `changed`, partial sums, sums and counts must EQUAL the reference, ties included.  REAL: Gaussian
blobs; labels must equal the reference on every point that is not within the worst-case fp32 rounding of a tie (kmeans_oracle.e_step; at
most 2 % of the points, asserted for these seeds on the CPU in test_kmeans_oracle_cpu.py), and every sum is compared with an fp64 sum
formed from the DEVICE's labels under the bound of an m-term fp32 sum, |error| <= m 2^-24 sum|x|."""
import functools

import numpy as np
import pytest
import torch

import kmeans_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = O.U
NAMES = sorted(O.CASES)
KINDS = ["exact", "real"]
SENT = -7777.25                                   # no sum of the test data: a partial that still holds it was not written
STATE = ("centers", "cnorm", "done", "labels", "psums", "pcounts", "sums", "counts", "changed", "tol", "n_iter", "scratch", "ticket", "ub", "lb",
         "xnorm", "cshift")


class State:
    """the buffers kmeans_lloyd_batched keeps for one batch, and the eight entry points on them"""

    def __init__(self, c):
        from partdistillation_amd import lib
        self.lib, self.L = lib, lib.load()
        self.sizes, self.C, self.K = list(c["sizes"]), c["C"], c["K"]
        self.B, self.N = len(self.sizes), int(sum(self.sizes))
        blocks, ranges = O.make_tables(self.sizes, c["slab"])
        self.blocks_np, self.ranges_np, self.nb = blocks, ranges, len(blocks)
        self.X = torch.from_numpy(c["X"].copy()).to(DEV)
        self.blocks, self.ranges = torch.from_numpy(blocks).to(DEV), torch.from_numpy(ranges).to(DEV)
        B, K, C, N = self.B, self.K, self.C, self.N
        self.centers = torch.from_numpy(c["centers"].copy()).to(DEV)
        self.cnorm = torch.from_numpy(c["cnorm"].copy()).to(DEV)
        self.done = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.labels = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        self.psums = torch.full((self.nb, K, C), SENT, dtype=torch.float32, device=DEV)
        self.pcounts = torch.full((self.nb, K), SENT, dtype=torch.float32, device=DEV)
        self.sums = torch.zeros((B, K, C), dtype=torch.float32, device=DEV)
        self.counts = torch.zeros((B, K), dtype=torch.float32, device=DEV)
        self.changed = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.tol = torch.zeros(B, dtype=torch.float32, device=DEV)
        self.n_iter = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.scratch = torch.full((int(self.L.pd_kmeans_reduce_update_scratch_floats(B, K, C)),), float("nan"), dtype=torch.float32, device=DEV)
        self.ticket = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.ub, self.lb, self.xnorm = (torch.full((N,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(3))
        self.cshift = torch.zeros((B, 2, 8), dtype=torch.float32, device=DEV)

    def clone(self):
        s = object.__new__(State)
        s.__dict__.update(self.__dict__)
        for f in STATE:
            setattr(s, f, getattr(self, f).clone())
        return s

    def _p(self, *names):
        return [getattr(self, n).data_ptr() for n in names]

    def _st(self):
        return self.lib.current_stream()

    def assign_atomic(self):
        self.lib.check(self.L.pd_kmeans_assign(*self._p("X", "blocks"), self.nb, *self._p("centers", "cnorm", "done", "labels", "sums", "counts", "changed"),
                                               self.C, self.K, self._st()))

    def assign_partial(self):
        self.lib.check(self.L.pd_kmeans_assign_partial(*self._p("X", "blocks"), self.nb,
                                                       *self._p("centers", "cnorm", "done", "labels", "psums", "pcounts", "changed"), self.C, self.K, self._st()))

    def assign_bounded(self):
        self.lib.check(self.L.pd_kmeans_assign_bounded(*self._p("X", "blocks"), self.nb,
                                                       *self._p("centers", "cnorm", "done", "labels", "psums", "pcounts", "changed", "ub", "lb", "xnorm", "cshift"),
                                                       self.C, self.K, self._st()))

    def reduce(self):
        self.lib.check(self.L.pd_kmeans_reduce(*self._p("psums", "pcounts", "ranges", "done", "sums", "counts"), self.B, self.K, self.C, self._st()))

    def update(self):
        self.lib.check(self.L.pd_kmeans_update(*self._p("centers", "cnorm", "sums", "counts", "changed", "tol", "done", "n_iter"), self.B, self.K, self.C,
                                               self._st()))

    def reduce_update(self):
        self.lib.check(self.L.pd_kmeans_reduce_update(*self._p("psums", "pcounts", "ranges", "centers", "cnorm", "changed", "tol", "done", "n_iter", "scratch",
                                                               "ticket"), self.B, self.K, self.C, self._st()))

    def reduce_update_shift(self):
        self.lib.check(self.L.pd_kmeans_reduce_update_shift(*self._p("psums", "pcounts", "ranges", "centers", "cnorm", "changed", "tol", "done", "n_iter",
                                                                     "scratch", "ticket", "cshift"), self.B, self.K, self.C, self._st()))

    def np(self, name):
        return getattr(self, name).cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """the data of a case and its first E-step in fp64 (computed once, shared, never written to)"""
    c = O.make_case(name, kind)
    c["scores"], c["ref_labels"], c["near"] = O.e_step(c["X"], c["centers"], c["cnorm"], c["img"])
    c["blocks"] = O.make_tables(c["sizes"], c["slab"])[0]
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def assert_labels(got, c, kind, what):
    if kind == "exact":
        assert np.array_equal(got, c["ref_labels"]), what
    else:
        ok = ~c["near"]
        assert (~ok).mean() <= O.NEAR_TIE_CAP
        assert np.array_equal(got[ok], c["ref_labels"][ok]), (what, np.flatnonzero(got[ok] != c["ref_labels"][ok])[:8])


def assert_sum(got, ref, abs_ref, m, kind, what):
    """a sum of at most m fp32 terms in any order against the fp64 sum: |error| <= (m - 1) u sum|x| (+ higher orders: m u is used)"""
    if kind == "exact":
        assert np.array_equal(got.astype(np.float64), ref), what
    else:
        assert (np.abs(got.astype(np.float64) - ref) <= m * U * abs_ref).all(), (what, float(np.abs(got - ref).max()))


def slab_npts(c):
    return c["blocks"][:, 2].astype(np.float64)[:, None, None]


# ---- 1. the E-step, three variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_e_step_three_variants_one_call(name, kind):
    """pd_kmeans_assign_partial, pd_kmeans_assign (atomics) and pd_kmeans_assign_bounded from a fresh state (labels -1, zero cshift), then a second
    call with the same centres.  Case c (K = 8, C = 2048) asks for 65,796 / 66,056 bytes of dynamic LDS, over 64 KiB, without
    hipFuncAttributeMaxDynamicSharedMemorySize being set (see test_lds_corner_k8_c2040_to_2048)."""
    c = case(name, kind)
    sp = State(c)
    sa, sb = sp.clone(), sp.clone()
    sp.assign_partial(), sa.assign_atomic(), sb.assign_bounded()
    torch.cuda.synchronize()
    lp, la, lb_ = sp.np("labels"), sa.np("labels"), sb.np("labels")
    assert_labels(lp, c, kind, "partial")
    assert np.array_equal(lp, la) and np.array_equal(lp, lb_)
    for s in (sp, sa, sb):
        assert s.np("changed").tolist() == c["sizes"]                                        # every label was -1
    assert torch.equal(sp.psums, sb.psums) and torch.equal(sp.pcounts, sb.pcounts)          # bit-identical
    m = O.m_step(c["X"], lp, c["centers"], c["img"], c["blocks"])                            # fp64 sums of the DEVICE's labels: pass B on its own
    assert np.array_equal(sp.np("pcounts").astype(np.float64), m["slab_counts"])
    assert np.array_equal(sa.np("counts").astype(np.float64), m["counts"])
    assert_sum(sp.np("psums"), m["slab_sums"], m["slab_abs"], slab_npts(c), kind, "slab sums")
    assert_sum(sa.np("sums"), m["sums"], m["abs_sums"], np.asarray(c["sizes"], np.float64)[:, None, None], kind, "atomic sums")
    if kind == "exact":                                                                      # the atomic sums are the reduced partials
        red = np.stack([sp.np("psums").astype(np.float64)[f:f + n].sum(0) for f, n in sp.ranges_np])
        assert np.array_equal(sa.np("sums").astype(np.float64), red)
    # second call, same centres: nothing changes
    keep = sp.psums.clone()
    for s in (sp, sa, sb):
        s.changed.zero_()
    sa.sums.zero_(), sa.counts.zero_()
    sp.assign_partial(), sa.assign_atomic(), sb.assign_bounded()
    torch.cuda.synchronize()
    for s in (sp, sa, sb):
        assert s.np("changed").tolist() == [0] * len(c["sizes"])
        assert np.array_equal(s.np("labels"), lp)
    assert torch.equal(sp.psums, keep) and torch.equal(sb.psums, keep) and torch.equal(sp.pcounts, sb.pcounts)


def test_lds_corner_k8_c2040_to_2048():
    """K = 8 with C >= 2040 needs more than 64 KiB of dynamic LDS ((8 C + 65) * 4 bytes; the bounded kernel 260 bytes more).  The limit the
    device reports (hipDeviceAttributeMaxSharedMemoryPerBlock, printed here) is 163,840 bytes on the MI355X, the 160 KiB of a CDNA4 compute unit:
    the launches are accepted without hipFuncAttributeMaxDynamicSharedMemorySize, and at the corner sizes they must compute the exact result, so
    the documented limit C <= 2048 at K = 8 stands."""
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    print(f"hipDeviceAttributeMaxSharedMemoryPerBlock = {limit}")
    assert limit >= (8 * 2048 + 64 + 64 + 2) * 4                                             # the bounded kernel's request at the corner
    rng = np.random.default_rng(2040)
    for C in (2040, 2044, 2048):
        X = rng.integers(-4, 5, size=(40, C)).astype(np.float32)
        centers = X[None, rng.choice(40, 8, replace=False)].copy()
        c = dict(sizes=[40], C=C, K=8, slab=32, X=X, centers=centers, cnorm=(centers.astype(np.float64) ** 2).sum(-1).astype(np.float32))
        ref = O.e_step(X, centers, c["cnorm"], np.zeros(40, dtype=np.int64))[1]
        sp = State(c)
        sa, sb = sp.clone(), sp.clone()
        sp.assign_partial(), sa.assign_atomic(), sb.assign_bounded()
        torch.cuda.synchronize()
        for s in (sp, sa, sb):
            assert np.array_equal(s.np("labels"), ref), C
        assert torch.equal(sp.psums, sb.psums)
        m = O.m_step(X, ref, centers, np.zeros(40, dtype=np.int64))
        assert np.array_equal(sa.np("sums").astype(np.float64), m["sums"]), C


# ---- 2. ties and empty clusters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dup", [(3, (1, 2)), (4, (0, 3)), (8, (2, 6))])
def test_duplicate_centres_lower_index_wins_and_empty_cluster_keeps_its_centre(K, dup):
    rng = np.random.default_rng(40 + K)
    C, n = 8, 70
    centers = rng.integers(-4, 5, size=(1, K, C)).astype(np.float32)
    while len(np.unique(centers[0], axis=0)) < K:
        centers = rng.integers(-4, 5, size=(1, K, C)).astype(np.float32)
    centers[0, dup[1]] = centers[0, dup[0]]
    X = np.clip(centers[0, rng.integers(K, size=n)] + rng.integers(-1, 2, size=(n, C)), -4, 4).astype(np.float32)
    c = dict(sizes=[n], C=C, K=K, slab=32, X=X, centers=centers, cnorm=(centers.astype(np.float64) ** 2).sum(-1).astype(np.float32))
    img = np.zeros(n, dtype=np.int64)
    ref = O.e_step(X, centers, c["cnorm"], img)[1]
    assert (ref == dup[0]).sum() > 5 and (ref == dup[1]).sum() == 0                          # the test's own premise
    m = O.m_step(X, ref, centers, img)
    want = np.where(m["counts"][..., None] > 0, m["sums"].astype(np.float32) / np.maximum(m["counts"], 1).astype(np.float32)[..., None], centers)
    base = State(c)
    for assign, finish in (("assign_partial", ("reduce_update",)), ("assign_bounded", ("reduce_update_shift",)), ("assign_atomic", ("update",)),
                           ("assign_partial", ("reduce", "update"))):
        s = base.clone()
        getattr(s, assign)()
        torch.cuda.synchronize()
        assert np.array_equal(s.np("labels"), ref), assign
        if assign != "assign_atomic":
            assert s.np("pcounts")[:, dup[1]].tolist() == [0.0] * s.nb
        for f in finish:
            getattr(s, f)()
        torch.cuda.synchronize()
        got = s.np("centers")
        assert np.array_equal(got[0, dup[1]], centers[0, dup[1]]) and s.np("cnorm")[0, dup[1]] == c["cnorm"][0, dup[1]], (assign, finish)
        assert np.array_equal(got, want), (assign, finish)                                    # sum / count: one correctly rounded fp32 division


def test_points_equidistant_from_two_distinct_centres_take_the_first():
    """centres 1 and 2 mirror each other in channel 0; points with x_0 = 0 have the same score for both (exactly), centre 0 and 3 are far"""
    C, K, n = 12, 4, 40
    rng = np.random.default_rng(9)
    centers = np.zeros((1, K, C), dtype=np.float32)
    centers[0, 0], centers[0, 3] = 4, -4
    centers[0, 1, 1:] = centers[0, 2, 1:] = rng.integers(-1, 2, size=C - 1)
    centers[0, 1, 0], centers[0, 2, 0] = -3, 3
    X = np.clip(centers[0, 1][None] + rng.integers(-1, 2, size=(n, C)), -4, 4).astype(np.float32)
    X[:, 0] = np.where(np.arange(n) % 3 == 0, 1.0, 0.0)                                      # every third point is nearer to centre 2
    c = dict(sizes=[n], C=C, K=K, slab=32, X=X, centers=centers, cnorm=(centers.astype(np.float64) ** 2).sum(-1).astype(np.float32))
    scores, ref, _ = O.e_step(X, centers, c["cnorm"], np.zeros(n, dtype=np.int64))
    tie = np.arange(n) % 3 != 0
    assert (scores[tie, 1] == scores[tie, 2]).all() and (ref[tie] == 1).all() and (ref[~tie] == 2).all()
    for assign in ("assign_partial", "assign_atomic", "assign_bounded"):
        s = State(c)
        getattr(s, assign)()
        torch.cuda.synchronize()
        assert np.array_equal(s.np("labels"), ref), assign


# ---- 3. reduce + update against reduce_update -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_reduce_and_update_against_reduce_update(name, kind):
    c = case(name, kind)
    base = State(c)
    base.assign_partial()
    torch.cuda.synchronize()
    labels = base.np("labels")
    m = O.m_step(c["X"], labels, c["centers"], c["img"], c["blocks"])
    n_slabs = base.ranges_np[:, 1].astype(np.float64)[:, None, None]
    two, one = base.clone(), base.clone()
    two.reduce()
    torch.cuda.synchronize()
    assert_sum(base.np("psums"), m["slab_sums"], m["slab_abs"], slab_npts(c), kind, "slab sums")
    assert np.array_equal(two.np("counts").astype(np.float64), m["counts"])
    # reduced sums: a slab sum of <= slab terms, then <= n_slabs + 7 additions (eight chains and their tree)
    assert_sum(two.np("sums"), m["sums"], m["abs_sums"], c["slab"] + n_slabs + 7, kind, "reduced sums")
    two.update(), one.reduce_update()
    rerun = base.clone()
    rerun.reduce_update()
    torch.cuda.synchronize()
    for f in ("centers", "cnorm", "done", "n_iter", "changed", "ticket", "scratch"):          # every sum in a fixed order
        assert torch.equal(getattr(one, f).view(torch.int32), getattr(rerun, f).view(torch.int32)), f
    assert not two.sums.any() and not two.counts.any()                                       # cleared for the next pd_kmeans_assign
    for s, what in ((two, "reduce + update"), (one, "reduce_update")):
        assert s.np("n_iter").tolist() == [1] * s.B and s.np("changed").tolist() == [0] * s.B and s.np("ticket").tolist() == [0] * s.B, what
        got, gn = s.np("centers"), s.np("cnorm")
        empty = m["counts"] == 0
        assert np.array_equal(got[empty], c["centers"][empty]), what
        if kind == "exact":
            want = np.where(empty[..., None], c["centers"], m["sums"].astype(np.float32) / np.maximum(m["counts"], 1).astype(np.float32)[..., None])
            assert np.array_equal(got, want), what                                           # 0 ulp: one correctly rounded division of exact operands
        else:
            bound = (n_slabs + 66) * U * m["abs_sums"] / np.maximum(m["counts"], 1)[..., None]
            assert (np.abs(got.astype(np.float64) - m["centers"]) <= bound).all(), (what, float((np.abs(got - m["centers"]) - bound).max()))
        c2 = (got.astype(np.float64) ** 2).sum(-1)
        assert (np.abs(gn.astype(np.float64) - c2) <= (c["C"] + 2) * U * c2).all(), what
    if kind == "exact":
        assert torch.equal(one.centers, two.centers)


# ---- 4. the convergence decision ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_convergence_decision_and_centre_shifts(name, kind):
    """done = (changed == 0) || (squared shift <= tol), for both update kernels, the true squared shift s from the fp64 M-step of the device's
    labels; cshift[b, 0, k] >= the move of centre k, cshift[b, 1, k] >= the largest move of another centre (they feed distance bounds, so never
    below), and neither more than 0.1 % above."""
    c = case(name, kind)
    base = State(c)
    base.assign_partial()
    torch.cuda.synchronize()
    assert base.np("changed").tolist() == c["sizes"]
    m = O.m_step(c["X"], base.np("labels"), c["centers"], c["img"])
    s = m["shift"]
    assert (s > 0).sum() >= 1
    for tol, zero_changed, table in ((0.5 * s, False, 0), (2.0 * s, False, 1), (0.0 * s, True, 1)):
        # the header's rule in fp64; the table's value wherever the centres move at all (an image whose only point IS its centre has s = 0)
        want = [int(zero_changed or s[b] <= tol[b]) for b in range(base.B)]
        assert all(w == table for w, sb in zip(want, s) if sb > 0)
        for path in ("reduce_update", "reduce+update", "reduce_update_shift"):
            st = base.clone()
            st.tol.copy_(torch.from_numpy(tol.astype(np.float32)))
            if zero_changed:
                st.changed.zero_()
            if path == "reduce+update":
                st.reduce(), st.update()
            else:
                getattr(st, path)()
            torch.cuda.synchronize()
            assert st.np("done").tolist() == want, (path, tol, zero_changed)
            assert st.np("n_iter").tolist() == [1] * st.B and st.np("changed").tolist() == [0] * st.B and st.np("ticket").tolist() == [0] * st.B
            if path == "reduce_update_shift":
                mv = np.sqrt(((st.np("centers").astype(np.float64) - c["centers"].astype(np.float64)) ** 2).sum(-1))     # [B, K], the device's own centres
                cs = st.np("cshift").astype(np.float64)
                for k in range(c["K"]):
                    other = np.delete(mv, k, axis=1).max(1) if c["K"] > 1 else np.zeros(st.B)
                    for row, mk in ((0, mv[:, k]), (1, other)):
                        assert (cs[:, row, k] >= mk).all() and (cs[:, row, k] <= 1.001 * mk + 1e-30).all(), (k, row, cs[:, row, k], mk)
                assert not cs[:, :, c["K"]:].any()


# ---- 5. done masking ------------------------------------------------------------------------------------------------------------------------------
def _three_images(K, C, seed):
    """whole numbers: the sums of the atomic path do not depend on the order of the atomics then, so every path can be compared bit for bit"""
    rng = np.random.default_rng(seed)
    sizes, Xs = [70, 45, 33], []
    for n in sizes:
        blobs = rng.integers(-3, 4, size=(K, C))
        Xs.append(np.clip(blobs[rng.integers(K, size=n)] + rng.integers(-1, 2, size=(n, C)), -4, 4).astype(np.float32))
    centers = np.stack([x[rng.choice(len(x), K, replace=False)] for x in Xs])
    return sizes, Xs, centers


@pytest.mark.parametrize("K,C", [(4, 260), (8, 64)])
def test_a_finished_image_is_left_untouched(K, C):
    """done = [0, 1, 0]: after one iteration of each path everything image 1 owns still holds its sentinel, and images 0 and 2 are what a batch
    without image 1 gives"""
    sizes, Xs, centers = _three_images(K, C, 50 + K)
    mk = lambda idx: dict(sizes=[sizes[i] for i in idx], C=C, K=K, slab=32, X=np.concatenate([Xs[i] for i in idx]), centers=centers[idx].copy(),
                          cnorm=(centers[idx].astype(np.float64) ** 2).sum(-1).astype(np.float32))
    full, pair = State(mk([0, 1, 2])), State(mk([0, 2]))
    p1 = slice(sizes[0], sizes[0] + sizes[1])                                                # points, slabs of image 1
    f1, n1 = full.ranges_np[1]
    s1 = slice(int(f1), int(f1 + n1))
    full.done[1] = 1
    full.labels[p1], full.centers[1], full.cnorm[1], full.n_iter[1], full.changed[1] = 5, 1234.5, -3.25, 77, 55
    full.psums[s1], full.pcounts[s1], full.sums[1], full.counts[1] = SENT, -9.5, 4321.0, 17.5
    full.ub[p1], full.lb[p1], full.xnorm[p1], full.cshift[1] = 0.5, 1.5, 2.5, 0.125
    full.tol[:], pair.tol[:] = 1e-4, 1e-4
    per_point = ("labels", "ub", "lb", "xnorm")
    per_slab = ("psums", "pcounts")
    per_image = ("centers", "cnorm", "n_iter", "changed", "sums", "counts", "cshift", "done", "ticket")

    def image1(s):
        return [getattr(s, f)[p1].clone() for f in per_point] + [getattr(s, f)[s1].clone() for f in per_slab] + [getattr(s, f)[1].clone() for f in per_image]

    before = image1(full)
    others_pts = np.r_[0:sizes[0], sizes[0] + sizes[1]:sum(sizes)]
    others_slabs = np.r_[0:int(f1), int(f1 + n1):full.nb]
    for path in (("assign_partial", "reduce_update"), ("assign_atomic", "update"), ("assign_bounded", "reduce_update_shift"), ("assign_partial", "reduce")):
        a, b = full.clone(), pair.clone()
        for call in path:
            getattr(a, call)(), getattr(b, call)()
        torch.cuda.synchronize()
        for x, y, f in zip(before, image1(a), per_point + per_slab + per_image):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (path, f)
        assert np.array_equal(a.np("labels")[others_pts], b.np("labels")), path
        for f in ("centers", "cnorm", "n_iter", "changed", "done", "sums", "counts", "ticket", "cshift"):
            assert np.array_equal(a.np(f)[[0, 2]].view(np.int32), b.np(f).view(np.int32)), (path, f)
        if path[0] != "assign_atomic":
            for f in per_slab:
                assert np.array_equal(a.np(f)[others_slabs].view(np.int32), b.np(f).view(np.int32)), (path, f)
        assert b.np("n_iter").tolist() == ([0, 0] if path[1] == "reduce" else [1, 1])


# ---- 6. the bounded path, iteration by iteration --------------------------------------------------------------------------------------------------
def _far_offset_run():
    """2000 points in FOUR channels around five blobs, everything moved 1000 units away from the origin: |x|^2 is 4 * 10^6, one fp32 unit in the
    last place of it is a tenth of the squared distance between a point and its centre, so d^2 = |x|^2 + score carries rounding errors as large
    as the gaps between the distances; and in four dimensions the centres often move straight towards a point, which makes the bounds tight.
    Only a skip margin that grows with |x|^2 + |c|^2 keeps the bounded E-step identical to the exhaustive one here (an fp32 emulation of both
    kernels with the margin set to zero leaves a stale label within 2 to 7 iterations for every seed tried).  Nearly every point is a near-tie by
    the reference's measure, so there is no comparison with it, and the fp32 run may cycle instead of ending: 16 iterations are stepped."""
    rng = np.random.default_rng(7100)
    C, K, n = 4, 4, 2000
    blobs = rng.normal(size=(K + 1, C)).astype(np.float32)
    X = (blobs[rng.integers(K + 1, size=n)] + rng.normal(size=(n, C)).astype(np.float32) + np.float32(1000.0)).astype(np.float32)
    centers = X[None, rng.choice(n, K, replace=False)].copy()
    return dict(sizes=[n], C=C, K=K, slab=32, X=X, centers=centers, cnorm=(centers.astype(np.float64) ** 2).sum(-1).astype(np.float32),
                img=np.zeros(n, dtype=np.int64))


@pytest.mark.parametrize("name", ["b", "g", "far"])
def test_bounded_path_iteration_by_iteration(name):
    """pd_kmeans_assign_bounded + pd_kmeans_reduce_update_shift against pd_kmeans_assign_partial + pd_kmeans_reduce_update, side by side (tol = 0: a
    run ends when no label changes): after EVERY iteration the same labels, changed counts, centres, norms, done flags and iteration counts bit for
    bit, and the bounded labels equal to the fp64 argmin for that iteration's centres, skipped points included.  In every iteration after the second
    the bounded call is also run on a copy whose partial sums hold a sentinel: a slab that keeps it was skipped, and the exhaustive path's partials of
    that slab must be the ones stored earlier.  `far`: see _far_offset_run."""
    far = name == "far"
    c = _far_offset_run() if far else O.make_run(name)
    bp, ep = State(c), State(c)
    kept_slabs, its, max_it = 0, 0, 16 if far else 60
    while its < max_it:
        cen, cn, live = bp.np("centers"), bp.np("cnorm"), bp.np("done")[c["img"]] == 0
        if its >= 2:
            probe = bp.clone()
            probe.psums.fill_(SENT)
        bp.assign_bounded(), ep.assign_partial()
        torch.cuda.synchronize()
        assert torch.equal(bp.labels, ep.labels) and torch.equal(bp.changed, ep.changed), its
        if not far:
            _, ref, near = O.e_step(c["X"], cen, cn, c["img"])
            assert near[live].mean() <= O.NEAR_TIE_CAP
            ok = live & ~near
            assert np.array_equal(bp.np("labels")[ok], ref[ok]), (its, np.flatnonzero(bp.np("labels")[ok] != ref[ok])[:8])
        if its >= 2:
            probe.assign_bounded()
            torch.cuda.synchronize()
            kept = (probe.psums == SENT).all(-1).all(-1) & (bp.done[bp.blocks[:, 0].long()] == 0)
            assert torch.equal(probe.labels, bp.labels)
            assert torch.equal(ep.psums[kept], bp.psums[kept]) and torch.equal(ep.pcounts[kept], bp.pcounts[kept]), its
            kept_slabs += int(kept.sum())
        bp.reduce_update_shift(), ep.reduce_update()
        torch.cuda.synchronize()
        its += 1
        for f in ("centers", "cnorm", "done", "n_iter", "changed", "ticket"):
            assert torch.equal(getattr(bp, f).view(torch.int32), getattr(ep, f).view(torch.int32)), (its, f)
        if bool(bp.done.all()):
            break
    assert bool(bp.done.all()) or far, "the run did not end"
    assert int(bp.n_iter.max()) >= 5
    if not far:
        assert kept_slabs > 0                                                                # the skip path ran


# ---- 7. limits and refusals -----------------------------------------------------------------------------------------------------------------------
def _small_state():
    c = case("a", "exact")
    s = State(c)
    s.assign_partial()
    torch.cuda.synchronize()
    return s


def _calls(s):
    """name -> (function, argument list, index of n_blocks / B, index of C, index of K, pointer indices)"""
    st = s._st()
    a7 = s._p("centers", "cnorm", "done", "labels")
    out = {
        "pd_kmeans_assign": [*s._p("X", "blocks"), s.nb, *a7, *s._p("sums", "counts", "changed"), s.C, s.K, st],
        "pd_kmeans_assign_partial": [*s._p("X", "blocks"), s.nb, *a7, *s._p("psums", "pcounts", "changed"), s.C, s.K, st],
        "pd_kmeans_assign_bounded": [*s._p("X", "blocks"), s.nb, *a7, *s._p("psums", "pcounts", "changed", "ub", "lb", "xnorm", "cshift"), s.C, s.K, st],
        "pd_kmeans_reduce": [*s._p("psums", "pcounts", "ranges", "done", "sums", "counts"), s.B, s.K, s.C, st],
        "pd_kmeans_update": [*s._p("centers", "cnorm", "sums", "counts", "changed", "tol", "done", "n_iter"), s.B, s.K, s.C, st],
        "pd_kmeans_reduce_update": [*s._p("psums", "pcounts", "ranges", "centers", "cnorm", "changed", "tol", "done", "n_iter", "scratch", "ticket"),
                                    s.B, s.K, s.C, st],
        "pd_kmeans_reduce_update_shift": [*s._p("psums", "pcounts", "ranges", "centers", "cnorm", "changed", "tol", "done", "n_iter", "scratch", "ticket"),
                                          None, s.B, s.K, s.C, st],
    }
    return out


def _layout(name, args):
    """positions of (count, C, K) in the argument list and of the pointers that must not be null"""
    n = len(args)
    if name.startswith("pd_kmeans_assign"):
        return 2, n - 3, n - 2, [i for i in range(n - 3) if i != 2]
    ptrs = [i for i in range(n - 4) if args[i] is not None]
    return n - 4, n - 2, n - 3, ptrs


def test_bad_arguments_are_refused_and_empty_launches_touch_nothing():
    s = _small_state()
    s.cshift.fill_(0.25)
    before = {f: getattr(s, f).clone() for f in STATE}
    for name, args in _calls(s).items():
        fn = getattr(s.L, name)
        i_n, i_c, i_k, ptrs = _layout(name, args)
        bad = [(i_c, 0), (i_k, 0), (i_k, 9), (i_n, -1)] + [(p, None) for p in ptrs]
        if name.startswith("pd_kmeans_assign"):
            bad += [(i_c, 6), (i_c, 2052)]
        for i, v in bad:
            a = list(args)
            a[i] = v
            with pytest.raises(s.lib.PdHipError):
                s.lib.check(fn(*a))
        a = list(args)
        a[i_n] = 0                                                                           # n_blocks = 0 / B = 0: OK, nothing launched
        s.lib.check(fn(*a))
    torch.cuda.synchronize()
    for f in STATE:
        assert torch.equal(getattr(s, f).view(torch.int32), before[f].view(torch.int32)), f


@pytest.mark.parametrize("B,K,C", [(1, 1, 4), (3, 2, 4), (2, 4, 260), (5, 5, 1028), (2, 8, 2048), (7, 3, 1536), (1, 4, 16), (1, 8, 8)])
def test_scratch_size_formula(B, K, C):
    from partdistillation_amd import lib
    assert lib.load().pd_kmeans_reduce_update_scratch_floats(B, K, C) == B * -(-(K * C) // 64) * (2 * (4 if K <= 4 else 8) + 1)
