"""Generate tests/golden/sem_criterion.npz: the reference's own semantic criterion on seeded logits, in float64.

Needs the reference tree (imported through oracle/ref_shim.py, nothing in it is edited):  python scripts/gen_sem_criterion_golden.py
The criterion is the one Model.__define_criterion builds and __minibatch applies (code/lib/model.py:102-133,255-269):
torch.nn.CrossEntropyLoss(weight) over the B*H*W pixels (labels = one-hot .max(1)), losses.dice.dice_loss(optimize_bg,
weight, smooth=1, time=1).  Stored per case: CE, Dice, and the autograd gradient of the criterion's sum
w.r.t. the logits as every GRAD_STRIDE-th element plus float64 checksums of the whole tensor (sum, sum of squares);
the inputs are re-made from the seed by `case_inputs`, which the tests import.
Cases: K in {2, 3, 5}, weights None / given, optimize_bg off / on, CE / Dice / Multi; B = 2 at 24 x 40.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

B, H, W = 2, 24, 40
OUT = os.path.join(ROOT, "tests", "golden", "sem_criterion.npz")
GRAD_STRIDE = 7


def case_inputs(i, K, weighted):
    """Seeded logits [B,K,H,W] float64, labels [B,H,W] int64, class weights [K] or None of case i."""
    rs = np.random.RandomState(1000 + i)
    logits = rs.standard_normal((B, K, H, W)) * 2.0
    labels = rs.randint(0, K, size=(B, H, W))
    weights = rs.uniform(0.2, 2.0, size=K) if weighted else None
    return logits, labels, weights


def cases():
    for K in (2, 3, 5):
        for weighted in (False, True):
            for bg in (False, True):
                for crit in ("CE", "Dice", "Multi"):
                    yield K, weighted, bg, crit


def main():
    import ref_shim
    ref_shim.install()
    from losses.dice import dice_loss
    out = {}
    for i, (K, weighted, bg, crit) in enumerate(cases()):
        logits, labels, weights = case_inputs(i, K, weighted)
        x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        onehot = torch.from_numpy(np.eye(K, dtype=np.int64)[labels]).permute(0, 3, 1, 2).contiguous()
        w = None if weights is None else torch.tensor(weights, dtype=torch.float64)
        cost = 0
        ce = dice = float("nan")
        if crit in ("CE", "Multi"):
            _, tgt = onehot.max(1)
            c = torch.nn.CrossEntropyLoss(w)(x.permute(0, 2, 3, 1).contiguous().view(-1, K), tgt.view(-1))
            cost = cost + c
            ce = float(c.detach())
        if crit in ("Dice", "Multi"):
            d = dice_loss(x, onehot, optimize_bg=bg, weight=w, smooth=1.0, time=1)
            cost = cost + d
            dice = float(d.detach())
        cost.backward()
        tag = "c%02d" % i
        out[tag + "/meta"] = np.array([K, int(weighted), int(bg), ("CE", "Dice", "Multi").index(crit)], dtype=np.int64)
        g = x.grad.numpy().reshape(-1)
        out[tag + "/ce"] = np.array(ce)
        out[tag + "/dice"] = np.array(dice)
        out[tag + "/grad_sub"] = g[::GRAD_STRIDE].copy()
        out[tag + "/grad_sums"] = np.array([g.sum(), (g * g).sum(), np.abs(g).sum()])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(list(cases())), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
