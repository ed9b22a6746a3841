"""CPU: a float64 restatement of the trainer's K-class semantic criterion and its gradient, pinned to the reference.

The restatement (`criterion`, `criterion_grad`) is the one the GPU tests hold the HIP kernels to.  It follows the
reference's definitions (Model.__define_criterion / __minibatch, code/lib/model.py:102-133,255-269; dice.py:10-85):
  CE   = sum_i w_{y_i} (lse_i - l_{y_i,i}) / sum_i w_{y_i}                       (CrossEntropyLoss(weight); w = 1: mean)
  D_bc = (2 sum p_c g_c + 1) / (sum p_c + sum g_c + 1)                           (time = 1, smooth = 1)
  Dice = mean_b (1 - mean_{c in C} w'_c D_bc),  C = 1..K-1 (0..K-1 with optimize_bg),  w' = |C| w_C / sum w_C  (or 1)
and the gradient w.r.t. the logits in closed form.  tests/golden/sem_criterion.npz holds the reference's own
dice_loss and CrossEntropyLoss, run in float64 with autograd (scripts/gen_sem_criterion_golden.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts")]

CRITERIA = ("CE", "Dice", "Multi")


def _softmax(logits):
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    s = e.sum(1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def _setup(logits, labels, weights, optimize_bg):
    B, K = logits.shape[:2]
    p, lse = _softmax(logits)
    g = (labels[:, None] == np.arange(K)[None, :, None, None]).astype(np.float64)
    w = np.ones(K) if weights is None else np.asarray(weights, dtype=np.float64)
    C = np.arange(0 if optimize_bg else 1, K)
    wn = np.zeros(K)
    wn[C] = len(C) * w[C] / w[C].sum()
    return p, lse, g, w, C, wn


def criterion(logits, labels, crit, weights=None, optimize_bg=False):
    """(CE, Dice) of float64 logits [B,K,H,W] against integer labels [B,H,W]; a term the criterion lacks is None."""
    p, lse, g, w, C, wn = _setup(logits, labels, weights, optimize_bg)
    ce = dice = None
    if crit in ("CE", "Multi"):
        wy = w[labels]
        ly = np.take_along_axis(logits, labels[:, None], 1)[:, 0]
        ce = float((wy * (lse - ly)).sum() / wy.sum())
    if crit in ("Dice", "Multi"):
        A, S, T = (p * g).sum((2, 3)), p.sum((2, 3)), g.sum((2, 3))
        D = (2 * A + 1) / (S + T + 1)
        dice = float((1 - (wn[None, C] * D[:, C]).mean(1)).mean())
    return ce, dice


def criterion_grad(logits, labels, crit, weights=None, optimize_bg=False):
    """d(CE + Dice)/d logits [B,K,H,W] (only the criterion's terms), closed form."""
    B, K = logits.shape[:2]
    p, lse, g, w, C, wn = _setup(logits, labels, weights, optimize_bg)
    out = np.zeros_like(logits)
    if crit in ("CE", "Multi"):
        wy = w[labels]
        out += (wy / wy.sum())[:, None] * (p - g)
    if crit in ("Dice", "Multi"):
        A, S, T = (p * g).sum((2, 3)), p.sum((2, 3)), g.sum((2, 3))
        den = S + T + 1
        coef = np.zeros((B, K))
        coef[:, C] = -wn[None, C] / (B * len(C))
        u = coef[:, :, None, None] * (2 * g / den[:, :, None, None] - ((2 * A + 1) / den ** 2)[:, :, None, None])
        out += p * (u - (p * u).sum(1, keepdims=True))
    return out


def golden_cases():
    from gen_sem_criterion_golden import case_inputs, GRAD_STRIDE
    z = np.load(os.path.join(ROOT, "tests", "golden", "sem_criterion.npz"))
    tags = sorted({k.split("/")[0] for k in z.files})
    for i, tag in enumerate(tags):
        K, weighted, bg, ci = (int(v) for v in z[tag + "/meta"])
        logits, labels, weights = case_inputs(i, K, bool(weighted))
        yield tag, dict(logits=logits, labels=labels, weights=weights, optimize_bg=bool(bg), crit=CRITERIA[ci],
                        ce=float(z[tag + "/ce"]), dice=float(z[tag + "/dice"]), grad_sub=z[tag + "/grad_sub"],
                        grad_sums=z[tag + "/grad_sums"], stride=GRAD_STRIDE)


def test_fixture_covers_the_issue_cases():
    seen = {(c["logits"].shape[1], c["weights"] is not None, c["optimize_bg"], c["crit"]) for _, c in golden_cases()}
    assert seen == {(K, wt, bg, cr) for K in (2, 3, 5) for wt in (False, True) for bg in (False, True) for cr in CRITERIA}


@pytest.mark.parametrize("tag,case", list(golden_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_restatement_matches_the_reference(tag, case):
    c = case
    ce, dice = criterion(c["logits"], c["labels"], c["crit"], c["weights"], c["optimize_bg"])
    if c["crit"] in ("CE", "Multi"):
        assert abs(ce - c["ce"]) <= 1e-12 * max(1.0, abs(c["ce"])), (ce, c["ce"])
    else:
        assert ce is None and np.isnan(c["ce"])
    if c["crit"] in ("Dice", "Multi"):
        assert abs(dice - c["dice"]) <= 1e-12 * max(1.0, abs(c["dice"])), (dice, c["dice"])
    else:
        assert dice is None and np.isnan(c["dice"])
    g = criterion_grad(c["logits"], c["labels"], c["crit"], c["weights"], c["optimize_bg"]).reshape(-1)
    ref = c["grad_sub"]
    assert np.abs(g[::c["stride"]] - ref).max() <= 1e-12 * np.abs(ref).max()
    sums = np.array([g.sum(), (g * g).sum(), np.abs(g).sum()])
    assert np.allclose(sums, c["grad_sums"], rtol=1e-12, atol=1e-14)


def test_weights_leave_two_class_fg_dice_unchanged():
    """At K = 2 without optimize_bg the one foreground weight normalises to 1 (w' = 1 * w_1 / w_1)."""
    rs = np.random.RandomState(5)
    logits, labels = rs.standard_normal((2, 2, 8, 8)), rs.randint(0, 2, (2, 8, 8))
    assert criterion(logits, labels, "Dice", [0.3, 3.0])[1] == pytest.approx(criterion(logits, labels, "Dice")[1], abs=1e-15)
    assert criterion(logits, labels, "CE", [0.3, 3.0])[0] != pytest.approx(criterion(logits, labels, "CE")[0])
