"""Writes tests/golden/cluster.npz: small embeddings, the initial centres of the deterministic maximin init, and the labels
of sklearn.cluster.KMeans(init=centres, n_init=1, algorithm='lloyd', tol=0, max_iter=iters) - the class the reference's
Prediction.cluster calls (code/lib/prediction.py:52-85) - run from those centres.  tests/test_cluster_ref.py pins the float64
restatement tests/cluster_np.py to these labels.  Needs scikit-learn (the fixture was made with 1.7.2)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import cluster_np as CN  # noqa: E402

# name: (H, W, C, instances, noise, separation, iters, seed)
CASES = {
    "overlap": (40, 52, 8, 6, 0.35, 1.2, 10, 3),
    "clear": (16, 12, 5, 3, 0.12, 3.0, 4, 5),
}


def sklearn_labels(x, fg, centres, iters):
    from sklearn.cluster import KMeans
    idx = np.flatnonzero(fg)
    km = KMeans(n_clusters=centres.shape[0], init=centres, n_init=1, algorithm='lloyd', tol=0, max_iter=iters)
    km.fit(x[idx])
    labels = np.zeros(x.shape[0], np.uint8)
    labels[idx] = km.labels_ + 1
    return labels


def main():
    import sklearn
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (H, W, C, n, noise, sep, iters, seed) in CASES.items():
        emb, fg, _ = CN.planted(1, H, W, C, n, seed, noise=noise, sep=sep)
        x = emb[0].reshape(C, H * W).T.astype(np.float64)
        f = fg[0].reshape(-1) != 0
        c0, _, _ = CN.farthest_init(x, f, n)
        out[name + ".emb"] = emb[0]
        out[name + ".fg"] = fg[0]
        out[name + ".init"] = c0
        out[name + ".iters"] = np.array(iters)
        out[name + ".labels"] = sklearn_labels(x, f, c0, iters).reshape(H, W)
    path = os.path.join(ROOT, "tests", "golden", "cluster.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
