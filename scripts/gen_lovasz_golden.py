"""Generate tests/golden/lovasz.npz: the reference's own lovasz_softmax on seeded logits, in fp32.

Needs the reference tree (imported through oracle/ref_shim.py, nothing in it is edited):  python scripts/gen_lovasz_golden.py
Per case the reference computes lovasz_softmax(softmax(x, 1), labels, only_present, per_image)
(code/lib/losses/lovasz_losses.py:156-196) on float32 logits, and autograd gives d loss / d x.  float32 because the
reference's own .float() casts make a float64 run raise in torch.dot.  Stored per case: the loss, every GRAD_STRIDE-th
element of the gradient, float64 checksums of the whole gradient (sum, sum of squares, sum of magnitudes); the inputs are
re-made from the seed by `case_inputs`, which the tests import.
Cases: K in {2, 3, 5}, per_image off / on, only_present off / on; B = 2 at 24 x 40.  The K = 5 cases have class 3 deleted
from the labels (an absent class counts with only_present off, and is skipped with it on).
The script also prints, per case, how far the float64 restatement (tests/lovasz_np.py) is from this fp32 run: the gap is
the reference's cancellation in jaccard[r] - jaccard[r-1], see tests/test_lovasz_ref.py.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

B, H, W = 2, 24, 40
OUT = os.path.join(ROOT, "tests", "golden", "lovasz.npz")
GRAD_STRIDE = 7
ABSENT = 3                       # the class deleted from the labels of the K = 5 cases


def cases():
    for K in (2, 3, 5):
        for per_image in (False, True):
            for only_present in (False, True):
                yield K, per_image, only_present


def case_inputs(i, K):
    """Seeded logits [B,K,H,W] float32 and labels [B,H,W] int64 of case i."""
    rs = np.random.RandomState(4000 + i)
    logits = (rs.standard_normal((B, K, H, W)) * 2.0).astype(np.float32)
    labels = rs.randint(0, K, size=(B, H, W))
    if K == 5:
        labels[labels == ABSENT] = 0
    return logits, labels


def main():
    import ref_shim
    ref_shim.install()
    from losses.lovasz_losses import lovasz_softmax as ref_lovasz
    from lovasz_np import lovasz_softmax
    out = {}
    for i, (K, per_image, only_present) in enumerate(cases()):
        logits, labels = case_inputs(i, K)
        x = torch.tensor(logits, dtype=torch.float32, requires_grad=True)
        loss = ref_lovasz(torch.softmax(x, 1), torch.from_numpy(labels), only_present=only_present, per_image=per_image)
        loss.backward()
        g = x.grad.numpy().astype(np.float64).reshape(-1)
        tag = "c%02d" % i
        out[tag + "/meta"] = np.array([K, int(per_image), int(only_present)], dtype=np.int64)
        out[tag + "/loss"] = np.array(float(loss.detach()))
        out[tag + "/grad_sub"] = g[::GRAD_STRIDE].copy()
        out[tag + "/grad_sums"] = np.array([g.sum(), (g * g).sum(), np.abs(g).sum()])
        ref = float(loss.detach())
        mine = lovasz_softmax(logits.astype(np.float64), labels, True, only_present, per_image)
        d = mine["grad"].reshape(-1) - g
        print("case %2d K=%d per_image=%d only_present=%d  loss rel %.2e  grad rel L2 %.2e" % (
            i, K, per_image, only_present, abs(mine["loss"] - ref) / abs(ref),
            np.sqrt((d * d).sum() / (g * g).sum())))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(list(cases())), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
