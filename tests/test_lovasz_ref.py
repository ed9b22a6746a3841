"""CPU: the float64 restatement of the Lovasz-Softmax criterion (tests/lovasz_np.py) pinned to the reference.

tests/golden/lovasz.npz holds the reference's own lovasz_softmax (code/lib/losses/lovasz_losses.py:156-196) on seeded
float32 logits, with autograd's gradient (scripts/gen_lovasz_golden.py; the reference cannot run in float64).  The
restatement, in float64 on the same float32 logits, must reproduce its loss within 1e-6 relative and its gradient within
1e-4 relative L2.  The gradient gap is the reference's, not the restatement's: lovasz_grad takes jaccard[r] - jaccard[r-1]
in float32, a difference of two numbers near 1 that are 1/U apart.  Measured when the fixture was generated (B = 2,
24 x 40; the generator prints them): loss 3.1e-9 .. 7.8e-8, gradient 1.5e-5 .. 4.6e-5 (batch-wide segments 2.6e-5 .. 4.6e-5,
per-image ones 1.5e-5 .. 2.3e-5).  In float64 the closed form and the Jaccard differences agree to 1e-12
(`test_closed_form_equals_jaccard_differences`)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import lovasz_np as R                     # noqa: E402
import gen_lovasz_golden as gen           # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lovasz.npz"))
CASES = list(enumerate(gen.cases()))


@pytest.mark.parametrize("i,case", CASES, ids=["K%d-img%d-present%d" % (k, p, o) for _, (k, p, o) in CASES])
def test_restatement_reproduces_the_reference(i, case):
    K, per_image, only_present = case
    tag = "c%02d" % i
    assert list(GOLD[tag + "/meta"]) == [K, int(per_image), int(only_present)]
    logits, labels = gen.case_inputs(i, K)
    if K == 5:
        assert not (labels == gen.ABSENT).any()
    got = R.lovasz_softmax(logits.astype(np.float64), labels, True, only_present, per_image)
    ref_loss = float(GOLD[tag + "/loss"])
    rel = abs(got["loss"] - ref_loss) / abs(ref_loss)
    g = got["grad"].reshape(-1)
    sub = GOLD[tag + "/grad_sub"]
    d = g[::gen.GRAD_STRIDE] - sub
    rel_g = float(np.sqrt((d * d).sum() / (sub * sub).sum()))
    sums = GOLD[tag + "/grad_sums"]
    print("case %d: loss rel %.2e, gradient rel L2 %.2e" % (i, rel, rel_g))
    assert rel <= 1e-6
    assert rel_g <= 1e-4
    # checksums of the whole gradient: sum of squares and of magnitudes (the plain sum is ~0: softmax gradients cancel)
    assert abs((g * g).sum() - sums[1]) <= 2e-4 * sums[1]
    assert abs(np.abs(g).sum() - sums[2]) <= 2e-4 * sums[2]
    assert abs(g.sum() - sums[0]) <= 1e-4 * sums[2]


@pytest.mark.parametrize("n,G", [(1, 0), (1, 1), (2, 1), (7, 0), (7, 7), (64, 20), (1000, 1), (1000, 999), (4097, 1500)])
def test_closed_form_equals_jaccard_differences(n, G):
    rs = np.random.RandomState(n * 31 + G)
    fg = np.zeros(n, dtype=np.int64)
    fg[rs.permutation(n)[:G]] = 1
    closed, diff = R.coefficients(fg), R.jaccard_differences(fg)
    assert closed.dtype == np.float64 and np.abs(closed - diff).max() <= 1e-12
    assert abs(closed.sum() - 1.0) <= 1e-12                       # the differences telescope to jaccard[n-1] = 1


def test_float32_jaccard_differences_cancel():
    """Why the kernels use the closed form: at 2^16 elements the float32 differences are 1e-3 off in relative L2."""
    rs = np.random.RandomState(5)
    fg = (rs.uniform(size=1 << 16) < 0.3).astype(np.int64)
    exact = R.coefficients(fg)
    f32 = R.jaccard_differences(fg, np.float32).astype(np.float64)
    assert np.linalg.norm(f32 - exact) / np.linalg.norm(exact) > 1e-4


def test_injected_order_and_ties():
    rs = np.random.RandomState(11)
    B, K, H, W = 2, 3, 5, 7
    logits = np.round(rs.standard_normal((B, K, H, W)) * 2) / 2           # coarse logits: many exact ties
    labels = rs.randint(0, K, size=(B, H, W))
    for per_image in (False, True):
        a = R.lovasz_softmax(logits, labels, True, False, per_image)
        b = R.lovasz_softmax(logits, labels, True, False, per_image, orders=a["orders"])
        assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"])
        e, o = a["errors"], a["orders"]
        for c in range(K):
            for s in range(e.shape[1]):
                es = e[c, s][o[c, s]]
                assert (np.diff(es) <= 0).all()
                tie = np.diff(es) == 0
                assert tie.any() and (np.diff(o[c, s])[tie] > 0).all()          # ties keep ascending pixel index


def test_options():
    rs = np.random.RandomState(3)
    B, K, H, W = 3, 4, 6, 5
    logits = rs.standard_normal((B, K, H, W)) * 2.5
    labels = rs.randint(0, K - 1, size=(B, H, W))                         # class K-1 absent
    labels[1] = 0                                                         # image 1 all background
    full = R.lovasz_softmax(logits, labels, True, False, True)
    sl, G = full["seg_loss"], full["G"]
    assert (G[K - 1] == 0).all() and (G[1:, 1] == 0).all()
    want = lambda keep: float(np.mean([sl[keep[:, s], s].mean() if keep[:, s].any() else 0.0 for s in range(B)]))
    allk = np.ones((K, B), dtype=bool)
    fgk = allk.copy(); fgk[0] = False
    assert abs(full["loss"] - want(allk)) < 1e-14
    assert abs(R.lovasz_softmax(logits, labels, False, False, True)["loss"] - want(fgk)) < 1e-14
    assert abs(R.lovasz_softmax(logits, labels, True, True, True)["loss"] - want(allk & (G > 0))) < 1e-14
    r = R.lovasz_softmax(logits, labels, False, True, True)
    assert abs(r["loss"] - want(fgk & (G > 0))) < 1e-14
    assert (r["grad"][1] == 0).all()                                      # no counted class in image 1: mean([]) == 0
    # numerical gradient of the loss at a few coordinates (the order is locally constant away from ties)
    base = R.lovasz_softmax(logits, labels, True, False, False)
    for idx in [(0, 0, 0, 0), (1, 2, 3, 4), (2, 3, 5, 1)]:
        h = 1e-6
        lp, lm = logits.copy(), logits.copy()
        lp[idx] += h; lm[idx] -= h
        num = (R.lovasz_softmax(lp, labels, True, False, False)["loss"] - R.lovasz_softmax(lm, labels, True, False, False)["loss"]) / (2 * h)
        assert abs(num - base["grad"][idx]) <= 1e-6 * max(1.0, abs(num)) + 1e-8
