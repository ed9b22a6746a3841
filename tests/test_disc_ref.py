"""CPU: the float64 restatement of the discriminative embedding loss (tests/disc_np.py) pinned to the reference.

tests/golden/disc.npz holds the reference's own functions (code/lib/losses/discriminative.py) on seeded float64 inputs with
autograd's gradients (scripts/gen_disc_golden.py).  Both sides are float64 and differ in summation order alone: every term
and both composed losses must agree to 1e-12 relative, the gradients to 1e-10 relative L2.  The rules for what the
reference leaves undefined (0/0) are checked against hand-computed values, the analytic gradient against central
differences."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import disc_np as R                       # noqa: E402
import gen_disc_golden as gen             # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "disc.npz"))
CASES = list(enumerate(gen.cases()))


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("i,case", CASES, ids=["B%d-%dx%d-norm%d" % (c[0], c[1], c[2], c[4]) for _, c in CASES])
def test_restatement_reproduces_the_reference(i, case):
    B, H, W, n_objects, norm = case
    tag = "c%02d/" % i
    assert list(GOLD[tag + "meta"]) == [B, H, W, norm] + list(n_objects)
    x, labels, _ = gen.case_inputs(i)
    dv, dd = gen.DELTAS[norm]
    assert all((labels[b] == k + 1).any() for b in range(B) for k in range(n_objects[b]))
    ref = R.form("reference", x, labels, n_objects, dv, dd, norm)
    full = R.form("full", x, labels, n_objects, dv, dd, norm)
    got = dict(ref_loss=ref["loss"], var_unit=ref["var"], qreg=ref["qreg"], full_loss=full["loss"], var_plain=full["var"],
               dist=full["dist"], reg=full["reg"])
    for key, v in got.items():
        r = rel(v, float(GOLD[tag + key]))
        print("case %d %s rel %.2e" % (i, key, r))
        assert float(GOLD[tag + key]) > 0 and r <= 1e-12, key
    for key, m in (("ref_means", ref["means"]), ("means_plain", full["means"])):
        want = GOLD[tag + key]
        assert want.shape == m.shape and np.linalg.norm(m - want) <= 1e-12 * np.linalg.norm(want), key
    for key, res in (("ref", ref), ("full", full)):
        g = res["grad"].reshape(-1)
        sub, sums = GOLD[tag + key + "_grad_sub"], GOLD[tag + key + "_grad_sums"]
        d = g[::gen.GRAD_STRIDE] - sub
        rg = float(np.sqrt((d * d).sum() / (sub * sub).sum()))
        print("case %d %s gradient rel L2 %.2e" % (i, key, rg))
        assert rg <= 1e-10
        assert abs((g * g).sum() - sums[1]) <= 2e-10 * sums[1] and abs(np.abs(g).sum() - sums[2]) <= 2e-10 * sums[2]
        assert abs(g.sum() - sums[0]) <= 1e-10 * sums[2]


def test_fixture_records_the_fp32_gap_of_the_reference():
    for i, _ in CASES:
        for key in ("ref32_gap_loss", "ref32_gap_grad"):
            v = float(GOLD["c%02d/%s" % (i, key)])
            assert 0 < v < 1e-5, (i, key, v)                              # an fp32 run of the reference, not a second fp64 one


def _small(seed, B=2, H=5, W=6, C=4, nb=(3, 2)):
    rs = np.random.RandomState(seed)
    labels = np.stack([rs.randint(0, n + 1, size=(H, W)) for n in nb])
    for b, n in enumerate(nb):
        labels[b].flat[:n] = np.arange(1, n + 1)
    return rs.standard_normal((B, C, H, W)) * 0.7, labels


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("name", ["reference", "full"])
def test_analytic_gradient_equals_central_differences(norm, name):
    x, labels = _small(3 + norm)
    dv, dd = (0.9, 1.2) if norm == 2 else (2.0, 2.5)
    unit, w = R.FORMS[name]
    w = tuple(v if v else 0.05 for v in w)                                # every term takes part in both forms
    base = R.discriminative(x, labels, (3, 2), dv, dd, norm, unit, w)
    assert base["var"] > 0 and base["dist"] > 0 and base["reg"] > 0 and base["qreg"] > 0
    for idx in [(0, 0, 0, 0), (0, 3, 2, 5), (1, 1, 4, 4), (1, 2, 0, 1), (0, 2, 3, 3)]:
        h = 1e-6
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        num = (R.discriminative(xp, labels, (3, 2), dv, dd, norm, unit, w)["loss"] -
               R.discriminative(xm, labels, (3, 2), dv, dd, norm, unit, w)["loss"]) / (2 * h)
        assert abs(num - base["grad"][idx]) <= 1e-6 * max(1.0, abs(num)) + 1e-8, (idx, num, base["grad"][idx])


@pytest.mark.parametrize("norm", [1, 2])
def test_empty_counted_instance_and_all_background_image(norm):
    """n_objects counts instance 2 of image 0, which has no pixel, and image 1 is all background: finite, and equal to the
    loss of the same data with the empty instance not counted and the background image contributing 0 to var / dist / reg
    (it still divides by B = 2) and its pixels' constant 1 to qreg."""
    x, labels = _small(11, nb=(2, 0))
    labels[1] = 0
    w = (1.0, 0.7, 0.3, 0.2)
    got = R.discriminative(x, labels, (3, 0), 0.4, 2.0, norm, False, w)
    assert all(np.isfinite(got[k]) for k in ("loss", "var", "dist", "reg", "qreg")) and np.isfinite(got["grad"]).all()
    assert got["n_present"] == 2 and (got["means"][0, 2] == 0).all() and (got["means"][1] == 0).all()
    one = R.discriminative(x[:1], labels[:1], (2,), 0.4, 2.0, norm, False, w)
    for k in ("var", "dist", "reg"):
        assert abs(got[k] - one[k] / 2) <= 1e-14 * max(1.0, abs(one[k])), k
    # by hand: the variance of image 0
    X = x[0].reshape(4, -1).T
    lab = labels[0].reshape(-1)
    F = int(((lab == 1) | (lab == 2)).sum())
    var = 0.0
    for i in (1, 2):
        d = X[lab == i] - X[lab == i].mean(0)
        nd = np.sqrt((d * d).sum(1)) if norm == 2 else np.abs(d).sum(1)
        var += (np.maximum(nd - 0.4, 0) ** 2).sum()
    assert abs(got["var"] - var / F / 2) <= 1e-14
    num = int((labels != 0).sum())
    fgn = np.sqrt((x * x).sum(1))[labels != 0]
    assert abs(got["qreg"] - (((fgn - 1) ** 2).sum() + (labels == 0).sum()) / num) <= 1e-13
    assert (got["grad"][1] == 0).all()                                    # background pixels carry no gradient
    # nothing anywhere: every term 0
    zero = R.discriminative(x, np.zeros_like(labels), (3, 2), 0.4, 2.0, norm, True, w)
    assert zero["loss"] == 0.0 and zero["qreg"] == 0.0 and (zero["grad"] == 0).all()


def test_planes_past_n_objects_are_foreground_for_qreg_only():
    x, labels = _small(5, nb=(3, 2))
    a = R.discriminative(x, labels, (2, 2), 0.4, 2.0, 2, False, (1, 1, 1, 1))
    cut = labels.copy()
    cut[0][cut[0] == 3] = 0
    b = R.discriminative(x, cut, (2, 2), 0.4, 2.0, 2, False, (1, 1, 1, 1))
    assert a["var"] == b["var"] and a["dist"] == b["dist"] and a["reg"] == b["reg"] and a["qreg"] != b["qreg"]
    assert a["num"] == b["num"] + int((labels[0] == 3).sum())


@pytest.mark.parametrize("norm", [1, 2])
def test_zero_difference_and_zero_mean(norm):
    """d = 0: a one-pixel instance sits on its own mean (plain means), and two instances share one mean; m = 0: an instance
    of two opposite pixels with unit means.  Everything stays finite and the rules give the hand-computed values."""
    C = 3
    x = np.zeros((1, C, 1, 6))
    labels = np.array([[[1, 2, 2, 3, 3, 0]]])
    x[0, :, 0, 0] = (0.5, -1.0, 2.0)                                      # instance 0: one pixel, d = 0
    x[0, :, 0, 1] = (1.0, 2.0, 0.0)                                       # instance 1: m = 0
    x[0, :, 0, 2] = (-1.0, -2.0, 0.0)
    x[0, :, 0, 3] = (0.5, -1.0, 2.0)                                      # instance 2: the mean of instance 0
    x[0, :, 0, 4] = (0.5, -1.0, 2.0)
    plain = R.discriminative(x, labels, (3,), 0.0, 1.0, norm, False, (1, 1, 0, 0))
    assert np.isfinite(plain["grad"]).all() and plain["n_present"] == 3
    n1 = np.sqrt(5.0) if norm == 2 else 3.0                               # |x - 0| of the two pixels of instance 1
    assert abs(plain["var"] - 2 * n1 * n1 / 5) <= 1e-14
    # the pair (0, 2) has distance 0: its hinge is the full margin, its direction 0
    d01 = np.sqrt(0.25 + 1 + 4) if norm == 2 else 3.5
    want = (2 * 2.0 ** 2 + 4 * max(2.0 - d01, 0.0) ** 2) / 6
    assert abs(plain["dist"] - want) <= 1e-14
    unit = R.discriminative(x, labels, (3,), 0.0, 1.0, norm, True, (1, 0, 1, 0))
    assert np.isfinite(unit["grad"]).all() and (unit["means"][0, 1] == 0).all()
    # instance 1 has mu = 0: its pixels keep the direct gradient only, 2 h / (B F) d|d|/dd with d = x
    px = x[0, :, 0, 1]
    direct = 2 * n1 / 5 * (px / np.sqrt(5.0) if norm == 2 else np.sign(px))
    assert np.abs(unit["grad"][0, :, 0, 1] - direct).max() <= 1e-14
