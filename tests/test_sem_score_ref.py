"""CPU-only: the numpy restatement of the semantic scoring rules (tests/sem_score_np.py) against independent brute-force
definitions - per-class loops over boolean masks -, evaluate.calc_dice for two classes, and the arg-max rules on
hand-made pixels."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sem_score_np as S        # noqa: E402
import evaluate as EV           # noqa: E402

INF, NAN = float("inf"), float("nan")


def brute_scores(labels, pred, K):
    """One image, straight from the definitions on boolean masks; labels >= K are left out."""
    labels, pred = labels.reshape(-1), pred.reshape(-1)
    ok = labels < K
    labels, pred = labels[ok], pred[ok]
    iou, dice = [], []
    for c in range(K):
        g, p = labels == c, pred == c
        union, inter = int((g | p).sum()), int((g & p).sum())
        iou.append(inter / union if union else NAN)
        dice.append(2 * inter / (int(g.sum()) + int(p.sum())) if union else NAN)
    present = [c for c in range(K) if not np.isnan(iou[c])]
    acc = float((labels == pred).sum()) / labels.size if labels.size else NAN
    miou = sum(iou[c] for c in present) / len(present) if present else NAN
    mdice = sum(dice[c] for c in present) / len(present) if present else NAN
    return np.array([acc, miou, mdice, len(present)] + iou + dice)


def same(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12, (got, want)


@pytest.mark.parametrize("K", [2, 3, 9, 32])
def test_confusion_and_scores_against_brute_force(K):
    rs = np.random.RandomState(K)
    n, L = 3, 500
    labels = rs.randint(0, K + 2, (n, L)).astype(np.uint8)            # some labels at and above K
    pred = rs.randint(0, K, (n, L)).astype(np.uint8)
    labels[1] = np.where(labels[1] == K - 1, 0, labels[1])            # image 1: class K-1 absent from the labels ...
    pred[1] = np.where(pred[1] == K - 1, 0, pred[1])                  # ... and from the prediction
    conf, oob = S.confusion(labels, pred, K)
    assert conf.dtype == np.int64 and conf.shape == (n, K, K)
    for i in range(n):
        for t in range(K):
            for p in range(K):
                assert conf[i, t, p] == int(((labels[i] == t) & (pred[i] == p)).sum())
        assert oob[i] == int((labels[i] >= K).sum()) and oob[i] > 0
        assert conf[i].sum() + oob[i] == L
        same(S.scores(conf[i]), brute_scores(labels[i], pred[i], K))
    got = S.scores(conf)
    assert got.shape == (n, 4 + 2 * K)
    assert np.isnan(got[1, 4 + K - 1]) and np.isnan(got[1, 4 + 2 * K - 1]) and got[1, 3] == K - 1
    # a dataset total is the score of the summed matrix, not the mean of the rows
    same(S.scores(conf.sum(0)), brute_scores(labels.reshape(-1), pred.reshape(-1), K))


def test_empty_and_diagonal_matrices():
    K = 4
    z = S.scores(np.zeros((K, K), np.int64))
    assert np.isnan(z[[0, 1, 2]]).all() and z[3] == 0 and np.isnan(z[4:]).all()
    d = S.scores(np.diag([5, 0, 7, 1 << 40]))
    assert d[0] == 1.0 and d[1] == 1.0 and d[2] == 1.0 and d[3] == 3
    assert np.isnan(d[5]) and np.isnan(d[4 + K + 1]) and (d[[4, 6, 7]] == 1.0).all()


def test_two_classes_dice_is_calc_dice():
    rs = np.random.RandomState(5)
    a = (rs.rand(4, 4096) < 0.3).astype(np.uint8)
    b = np.where(rs.rand(4, 4096) < 0.8, a, 1 - a).astype(np.uint8)
    conf, oob = S.confusion(a, b, 2)
    assert not oob.any()
    sc = S.scores(conf)
    for i in range(4):
        assert sc[i, 4 + 2 + 1] == EV.calc_dice(a[i] == 1, b[i] == 1)


def test_class_map_rules_on_hand_made_pixels():
    K, ld = 5, 8
    pad = [INF, NAN, INF]                                             # channels K..ld-1 never take part
    rows = [
        ([1.0, 3.0, 3.0, 2.0, 3.0], 1),                               # tie: the first maximum
        ([NAN, 9.0, 1.0, 2.0, 3.0], 0),                               # NaN first
        ([1.0, 9.0, 1.0, 2.0, NAN], 4),                               # NaN last: NaN is the maximum
        ([1.0, NAN, INF, NAN, 3.0], 1),                               # the first NaN, even against +inf
        ([-INF] * 5, 0),                                              # all -inf: class 0
        ([0.0, INF, 5.0, INF, 1.0], 1),                               # +inf tie
        ([-INF, -INF, -3.0, -INF, -INF], 2),
        ([-0.0, 0.0, -1.0, -1.0, -1.0], 0),                           # -0.0 == 0.0: a tie
    ]
    x = np.array([r + pad for r, _ in rows], np.float32)
    assert x.shape == (len(rows), ld)
    assert S.class_map(x, K).tolist() == [w for _, w in rows]
    assert S.class_map(x.reshape(2, 4, ld), K).shape == (2, 4)
    # the same rule as torch.argmax on the K channels
    import torch
    assert torch.argmax(torch.from_numpy(x[:, :K]), 1).tolist() == [w for _, w in rows]
