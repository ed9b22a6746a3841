"""CPU-only: the float64 restatement tests/cluster_np.py of the embedding clustering.  Its Lloyd iterations are pinned to
sklearn.cluster.KMeans - the class the reference's Prediction.cluster calls - through tests/golden/cluster.npz
(scripts/make_cluster_golden.py) and, when scikit-learn imports, through a live run; the mean-shift is checked on planted
partitions, on inputs built to stall it, and through its assign_rest / min_pixels / empty-foreground rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import cluster_np as CN  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cluster.npz"))
CASES = sorted({k.split(".")[0] for k in GOLD.files if "." in k})


def _case(name):
    emb, fg = GOLD[name + ".emb"], GOLD[name + ".fg"]
    C = emb.shape[0]
    return emb.reshape(C, -1).T.astype(np.float64), fg.reshape(-1) != 0, GOLD[name + ".init"], int(GOLD[name + ".iters"])


def _same_partition(a, b):
    """Two label vectors describe the same partition (labels may be numbered differently)."""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("name", CASES)
def test_lloyd_equals_the_sklearn_fixture(name):
    x, fg, init, iters = _case(name)
    r = CN.lloyd(x, fg, init, iters)
    assert np.array_equal(r["labels"], GOLD[name + ".labels"].reshape(-1))
    assert r["sizes"].min() > 0                            # the empty-cluster rule (sklearn relocates instead) never fired
    c0, _, _ = CN.farthest_init(x, fg, init.shape[0])
    assert np.array_equal(c0, init)                        # the fixture's centres are the maximin init's
    k = CN.kmeans(x, fg, init.shape[0], iters=iters)
    assert np.array_equal(k["labels"], r["labels"]) and k["n_objects"] == init.shape[0]


@pytest.mark.parametrize("name", CASES)
def test_lloyd_equals_a_live_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans
    x, fg, init, iters = _case(name)
    for it in (1, iters):
        km = KMeans(n_clusters=init.shape[0], init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=it).fit(x[fg])
        r = CN.lloyd(x, fg, init, it)
        assert np.array_equal(r["labels"][fg], km.labels_ + 1)
        assert np.abs(r["centres"] - km.cluster_centers_).max() < 1e-12


def test_lloyd_rules():
    x = np.array([[0.0, 0], [1, 0], [10, 0], [11, 0], [5.5, 0], [100, 100]])
    fg = np.array([1, 1, 1, 1, 1, 0], bool)
    cen = np.array([[0.0, 0], [11, 0], [50, 50]])
    r = CN.lloyd(x, fg, cen, 3)
    assert r["labels"].tolist() == [1, 1, 2, 2, 1, 0]      # the tie at 5.5 after the update goes to the lowest index
    assert np.array_equal(r["centres"][2], cen[2]) and r["sizes"].tolist() == [3, 2, 0]        # empty: keeps its centre
    assert CN.lloyd(x, fg, cen, 0)["moved"] == 0 and r["moved"] == 0
    assert CN.lloyd(x, fg, cen, 1)["moved"] == 0
    assert CN.kmeans(x, fg, 0)["labels"].tolist() == [0] * 6 and CN.kmeans(x, fg, 0)["n_objects"] == 0
    assert CN.kmeans(x, fg, 9)["n_objects"] == 5           # no more clusters than foreground pixels
    far = CN.farthest_init(x, fg, 3)
    assert far[1].tolist() == [0, 3, 4]                    # first pixel, the farthest, then the farthest from both


@pytest.mark.parametrize("seed,C,n", [(0, 24, 6), (1, 8, 3), (2, 32, 12)])
def test_meanshift_recovers_a_planted_partition(seed, C, n):
    emb, fg, truth = CN.planted(1, 24, 20, C, n, seed, noise=0.1)
    r = CN.cluster(emb, fg, 'meanshift', bandwidth=1.5)
    assert r["n_objects"][0] == n
    m = fg[0].reshape(-1) != 0
    assert _same_partition(r["labels"][0].reshape(-1)[m], truth[0].reshape(-1)[m])
    assert not r["labels"][0].reshape(-1)[~m].any()
    assert r["sizes"][0, :n].sum() == m.sum()
    k = CN.cluster(emb, fg, 'kmeans', n_objects=[n], iters=5)
    assert _same_partition(k["labels"][0].reshape(-1)[m], truth[0].reshape(-1)[m]) and k["moved"][0] == 0
    ref = CN.cluster(emb, fg, 'meanshift', bandwidth=1.5, refine=2)
    assert np.array_equal(ref["labels"], r["labels"])      # a clean partition is a fixed point of Lloyd


def test_meanshift_terminates_on_adversarial_input():
    fg = np.ones(50, bool)
    same = CN.meanshift(np.ones((50, 4)), fg, 1.0)
    assert same["n_objects"] == 1 and same["rounds"] == 1 and same["sizes"].tolist() == [50]
    far = 10.0 * np.arange(50, dtype=np.float64)[:, None] * np.ones((1, 4))     # every pixel beyond bw of every other
    r = CN.meanshift(far, fg, 1.0, assign_rest=False)
    assert r["n_objects"] == 32 and r["rounds"] == 32 and r["labels"].tolist() == list(range(1, 33)) + [0] * 18
    r = CN.meanshift(far, fg, 1.0, min_pixels=2, assign_rest=True, max_rounds=64)
    assert r["n_objects"] == 0 and r["rounds"] == 50 and not r["labels"].any()  # all noise, and nothing to assign it to
    r = CN.meanshift(far, fg, 1.0, min_pixels=2)                # the round budget: refused balls use it up (default 32)
    assert r["n_objects"] == 0 and r["rounds"] == 32 and not r["labels"].any()
    assert CN.meanshift(far, fg, 1.0, shifts=0, max_objects=3)["labels"].tolist() == [1, 2] + [3] * 48


def test_meanshift_round_budget_counts_refused_balls():
    rng = np.random.RandomState(8)
    a, b = 0.05 * rng.randn(20, 3), 0.05 * rng.randn(20, 3) + np.array([3.0, 0, 0])
    lone = np.array([[0.0, 9.0, 0.0]])
    x = np.concatenate([lone, a, b])                       # the first pixel is a lone outlier
    fg = np.ones(len(x), bool)
    r = CN.meanshift(x, fg, 0.5, max_objects=1, min_pixels=2)  # the only round goes to the refused ball
    assert r["n_objects"] == 0 and r["rounds"] == 1 and not r["labels"].any()
    r = CN.meanshift(x, fg, 0.5, max_objects=1, min_pixels=2, max_rounds=2)
    assert r["n_objects"] == 1 and r["rounds"] == 2 and r["labels"].tolist() == [1] * 41 and r["sizes"].tolist() == [20]
    r = CN.meanshift(x, fg, 0.5, max_objects=2, min_pixels=2, assign_rest=False)          # outlier, then a: b is not visited
    assert r["n_objects"] == 1 and r["rounds"] == 2 and r["labels"].tolist() == [0] + [1] * 20 + [0] * 20
    r = CN.meanshift(x, fg, 0.5, max_objects=2, min_pixels=2, assign_rest=False, max_rounds=3)
    assert r["n_objects"] == 2 and r["rounds"] == 3 and r["labels"].tolist() == [0] + [1] * 20 + [2] * 20
    with pytest.raises(AssertionError):
        CN.meanshift(x, fg, 0.5, max_objects=4, max_rounds=3)


def test_meanshift_assign_rest_and_noise():
    rng = np.random.RandomState(4)
    a, b = 0.05 * rng.randn(30, 3), 0.05 * rng.randn(20, 3) + np.array([3.0, 0, 0])
    lone = np.array([[1.4, 0.0, 0.0]])                     # nearer to cluster a, outside both balls
    x = np.concatenate([a[:10], lone, b, a[10:]])
    fg = np.ones(len(x), bool)
    on = CN.meanshift(x, fg, 0.5, min_pixels=5)
    off = CN.meanshift(x, fg, 0.5, min_pixels=5, assign_rest=False)
    assert on["n_objects"] == off["n_objects"] == 2 and on["sizes"].tolist() == off["sizes"].tolist() == [30, 20]
    assert off["labels"][10] == 0 and on["labels"][10] == 1
    assert np.array_equal(np.delete(on["labels"], 10), np.delete(off["labels"], 10))
    cap = CN.meanshift(x, fg, 0.5, max_objects=1)          # the cap: cluster b and the lone pixel go to the only centre
    assert cap["n_objects"] == 1 and cap["labels"].tolist() == [1] * len(x) and cap["sizes"].tolist() == [30]
    cap = CN.meanshift(x, fg, 0.5, max_objects=1, assign_rest=False)
    assert int((cap["labels"] == 0).sum()) == 21
    fg2 = fg.copy()
    fg2[:5] = False
    part = CN.meanshift(x, fg2, 0.5)
    assert not part["labels"][:5].any() and part["n_objects"] == 3 and part["sizes"].tolist() == [25, 1, 20]


def test_empty_foreground_and_batch_form():
    emb, fg, _ = CN.planted(2, 8, 12, 5, [0, 2], 7, noise=0.1)
    assert not fg[0].any()
    for r in (CN.cluster(emb, fg, 'meanshift', bandwidth=1.5), CN.cluster(emb, fg, 'kmeans', n_objects=[3, 2])):
        assert r["n_objects"].tolist() == [0, 2] and not r["labels"][0].any() and not r["centres"][0].any()
        assert r["labels"].shape == (2, 8, 12) and r["labels"].dtype == np.uint8 and r["centres"].shape == (2, 32, 5)
    r = CN.cluster(emb, fg, 'kmeans', n_objects=[3, 0])
    assert not r["labels"].any() and r["n_objects"].tolist() == [0, 0]
