"""The fp64 K-means step reference of the kernel tests (tests/kmeans_oracle.py) against two independent implementations — the
sklearn-pinned restatement oracle.proposal_generation_ref.kmeans_lloyd_np and scikit-learn itself — with injected initial centres;
and the share of near-tie points the GPU tests may leave out of a label comparison, for exactly the data they use."""
import numpy as np
import pytest

import kmeans_oracle as O
from oracle import proposal_generation_ref as P

BLOBS = [(83, 40, 4, 3), (500, 16, 4, 4), (40, 8, 3, 5)]            # N, C, K, seed


def _blobs(N, C, K, seed):
    rng = np.random.default_rng(seed)
    blobs = rng.normal(size=(K, C)).astype(np.float32) * 2
    X = (blobs[rng.integers(K, size=N)] + rng.normal(size=(N, C)).astype(np.float32)).astype(np.float32)
    return X, X[rng.choice(N, K, replace=False)].copy()


def _oracle_run(X, init, tol=1e-4):
    """sklearn's conventions around the header's loop: tol scaled by the mean per-feature variance; after a stop on tol the labels are
    those of the final centres"""
    centers, labels, n_iter, strict = O.lloyd(X, init, np.var(X.astype(np.float64), axis=0).mean() * tol)
    if not strict:
        labels = O.e_step(X, centers[None], (centers * centers).sum(-1)[None], np.zeros(len(X), dtype=np.int64))[1]
    return centers, labels, n_iter


@pytest.mark.parametrize("N,C,K,seed", BLOBS)
def test_oracle_lloyd_matches_the_sklearn_restatement(N, C, K, seed):
    X, init = _blobs(N, C, K, seed)
    centers, labels, n_iter = _oracle_run(X, init)
    c_ref, l_ref, it_ref = P.kmeans_lloyd_np(X, init)
    assert np.array_equal(labels, l_ref) and n_iter == it_ref
    assert np.abs(centers - c_ref).max() <= 1e-5


@pytest.mark.parametrize("N,C,K,seed", BLOBS)
def test_oracle_lloyd_matches_sklearn(N, C, K, seed):
    from sklearn.cluster import KMeans
    X, init = _blobs(N, C, K, seed)
    centers, labels, n_iter = _oracle_run(X, init)
    sk = KMeans(n_clusters=K, init=init, n_init=1, algorithm="lloyd").fit(X)
    assert np.array_equal(labels, sk.labels_) and n_iter == sk.n_iter_
    assert np.abs(centers - sk.cluster_centers_).max() <= 1e-5


def test_tables_are_those_of_the_product():
    blocks, ranges = O.make_tables([70, 1, 64, 9], 32)
    assert blocks.tolist() == [[0, 0, 32], [0, 32, 32], [0, 64, 6], [1, 70, 1], [2, 71, 32], [2, 103, 32], [3, 135, 9]]
    assert ranges.tolist() == [[0, 3], [3, 1], [4, 2], [6, 1]]
    assert blocks.dtype == np.int32 and ranges.dtype == np.int32


def test_e_step_first_minimum_and_m_step_empty_cluster():
    X = np.array([[0, 1.0], [0, -1.0], [3, 0]], dtype=np.float32)
    centers = np.array([[[1, 0], [-1, 0], [-1, 0.0]]], dtype=np.float32)          # points 0, 1 are equidistant from all three; 1 == 2
    scores, labels, near = O.e_step(X, centers, (centers ** 2).sum(-1), np.zeros(3, dtype=np.int64))
    assert labels.tolist() == [0, 0, 0] and near.tolist() == [True, True, False]
    assert np.array_equal(scores[0], [1.0, 1.0, 1.0])
    m = O.m_step(X, np.array([0, 0, 1]), centers, np.zeros(3, dtype=np.int64))
    assert m["counts"].tolist() == [[2, 1, 0]] and np.array_equal(m["centers"][0], [[0, 0], [3, 0], [-1, 0]])
    assert np.allclose(m["moves"], [[1.0, 4.0, 0.0]]) and np.allclose(m["shift"], [17.0]) and np.allclose(m["cnorm"], [[0, 9, 1]])


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_near_tie_share_of_the_real_cases(name):
    c = O.make_case(name, "real")
    near = O.e_step(c["X"], c["centers"], c["cnorm"], c["img"])[2]
    assert near.mean() <= O.NEAR_TIE_CAP, near.mean()


@pytest.mark.parametrize("name", ["b", "g"])
def test_near_tie_share_along_the_stepped_runs(name):
    """every iteration of the runs that the bounded E-step is stepped through (centres rounded to fp32 as the device stores them), which
    must also be long enough to be worth stepping"""
    c = O.make_run(name)
    centers, cnorm = c["centers"].copy(), c["cnorm"].copy()
    labels, done, n_iter = np.full(len(c["X"]), -1), np.zeros(len(c["sizes"]), dtype=bool), np.zeros(len(c["sizes"]), dtype=int)
    while not done.all() and n_iter.max() < 60:
        live = ~done[c["img"]]
        _, new, near = O.e_step(c["X"], centers, cnorm, c["img"])
        assert near[live].mean() <= O.NEAR_TIE_CAP
        changed = np.bincount(c["img"][live & (new != labels)], minlength=len(done))
        labels = np.where(live, new, labels)
        m = O.m_step(c["X"], labels, centers, c["img"])
        for b in np.flatnonzero(~done):
            centers[b] = m["centers"][b].astype(np.float32)
            cnorm[b] = (centers[b].astype(np.float64) ** 2).sum(-1).astype(np.float32)
            n_iter[b] += 1
            done[b] = changed[b] == 0
    assert done.all() and n_iter.max() >= 5, n_iter
