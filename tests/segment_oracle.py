"""The procedure of ReSeg.segment driven through the blocks of oracle/reseg_ref.py (helper module for
tests/test_segment_ref.py and tests/test_gpu_segment.py), and the lockstep comparison of a run of it ("the device":
the HIP path, or the float32 oracle in the CPU test) against the float64 oracle.

Lockstep: at every iteration the oracle decodes FROM THE DEVICE'S point and remaining set, so that one near-tie
cannot cascade.  With tol = 1e-3 - the whole-model fp32 forward bound tests/test_gpu_model.py applies to
attend.pro_merge and to every it%d.L%d tensor - relative to the oracle tensor's largest magnitude:
  (a) the device's merge (once) and level-4 pred (every iteration) are within tol of the oracle's;
  (b) the device's point p satisfies merge_oracle[p] >= max over remaining of merge_oracle - 2 * tol * max|merge|;
  (c) the device's claim equals the oracle's on every pixel whose oracle margin |l1 - l0| exceeds
      2 * tol * max|logit| (the rule assert_index_map applies to sem_argmax).
Conditions on the case, not measurements: the pixels (c) excuses are at most 1 % of the image's foreground in any
iteration; the iterations in which the device's point is not the oracle's own arg-max are at most 2 per image; in every
image at least one iteration claims 16 pixels or more."""
import numpy as np
import torch

import reseg_ref as R
import segment_np as S

TOL = 1e-3


class Oracle:
    """merge [B,L] and decode(s_t) -> level-4 logits [B,L,2] (float64 numpy) from the oracle's blocks in `dtype`,
    with `fg` (bool / {0,1} [B,H,W]) in the place of the predicted foreground."""

    def __init__(self, sd, x, fg, dtype=torch.float64):
        self.P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.ctx = R.Ctx()
        B, _, H, W = x.shape
        self.B, self.H, self.W = B, H, W
        with torch.no_grad():
            x_dec, self.feats = R.unet(self.P, x.to(dtype), self.ctx)
            x_enc = R.ins_stems(self.P, x_dec, self.ctx)
            self.sem_mask = torch.as_tensor(np.asarray(fg)).reshape(B, 1, H, W).to(dtype)
            s = R.spatial_attention(self.P, x_enc, self.sem_mask, self.ctx)
            _, merge = R.hard_attention(self.P, s, self.sem_mask, torch.ones(B, 1, H, W, dtype=dtype), self.ctx)
        self.merge = merge.reshape(B, -1).double().numpy()
        self.gold = torch.zeros(B, 1, H, W, dtype=dtype)

    def decode(self, s_t):
        rows, cols = [int(v) // self.W for v in s_t], [int(v) % self.W for v in s_t]
        with torch.no_grad():
            _, preds = R.pyramid_decoder(self.P, self.feats, rows, cols, self.sem_mask, self.gold, self.ctx, "seg")
        return preds[4].permute(0, 2, 3, 1).reshape(self.B, -1, 2).double().numpy()


def run_loop(oracle, fg, iters):
    """The procedure on an Oracle's own points.  Returns the record lockstep() takes as `dev`."""
    preds = []

    def decode(s_t):
        preds.append(oracle.decode(s_t))
        return preds[-1]
    fgf = np.asarray(fg).reshape(oracle.B, -1).astype(np.float32)
    labels, count, trace = S.segment_loop(fgf, oracle.merge, decode, iters)
    return dict(merge=oracle.merge, s_t=[t["s_t"] for t in trace], pred=preds, labels=labels, count=count)


def lockstep(dev, ref, fg, what, tol=TOL):
    """dev: dict(merge [B,L], s_t [T][B], pred [T][B,L,2], labels [B,L], count [B]); ref: the float64 Oracle.
    Asserts (a), (b), (c) and the three conditions; returns the measured figures."""
    B = ref.B
    fgf = np.asarray(fg).reshape(B, -1).astype(np.float32)
    fg_px = (fgf > 0.5).sum(1)
    mo = ref.merge
    e_merge = float(np.abs(np.asarray(dev["merge"], np.float64) - mo).max() / np.abs(mo).max())
    assert e_merge <= tol, (what, "merge", e_merge)
    st = S.seg_begin(fgf, dev["merge"])
    mism, biggest = np.zeros(B, int), np.zeros(B, int)
    e_pred, worst_gap, worst_excused = 0.0, 0.0, 0.0
    for t, (s_dev, p_dev) in enumerate(zip(dev["s_t"], dev["pred"])):
        s_dev = np.asarray(s_dev).astype(np.int64)
        remaining = (fgf > 0.5) & (st["labels"] == 0)
        active = remaining.any(1)
        for b in range(B):
            if not active[b]:
                continue
            assert remaining[b, s_dev[b]], (what, t, b, "the device's point is not a remaining pixel")
            best = mo[b][remaining[b]].max()
            gap = float((best - mo[b, s_dev[b]]) / np.abs(mo).max())
            worst_gap = max(worst_gap, gap)
            assert gap <= 2 * tol, (what, t, b, "point", gap)                                   # (b)
            mism[b] += int(S.masked_first_argmax(mo[b], remaining[b]) != s_dev[b])
        p_ref = ref.decode(s_dev)
        p_dev = np.asarray(p_dev, np.float64)
        e = float(np.abs(p_dev - p_ref).max() / np.abs(p_ref).max())
        e_pred = max(e_pred, e)
        assert e <= tol, (what, t, "pred", e)                                                   # (a)
        before = st["labels"].copy()
        count = st["count"].copy()
        S.seg_claim(st, p_dev, fgf, dev["merge"], s_dev)            # the device's own claim, restated
        thr = 2 * tol * float(np.abs(p_ref).max())
        for b in range(B):
            if not active[b]:
                assert np.array_equal(st["labels"][b], before[b]), (what, t, b, "inactive image relabelled")
                continue
            point = np.zeros(fgf.shape[1], bool)
            point[s_dev[b]] = True
            claim_ref = remaining[b] & ((p_ref[b, :, 1] > p_ref[b, :, 0]) | point)
            claim_dev = (st["labels"][b] == count[b] + 1) & (before[b] == 0)
            sure = (np.abs(p_ref[b, :, 1] - p_ref[b, :, 0]) > thr) | point
            bad = remaining[b] & sure & (claim_ref != claim_dev)
            assert not bad.any(), (what, t, b, "claim differs on %d confident pixels" % int(bad.sum()))   # (c)
            excused = float((remaining[b] & ~sure).sum()) / max(int(fg_px[b]), 1)
            worst_excused = max(worst_excused, excused)
            assert excused <= 0.01, (what, t, b, "excused share", excused)
            biggest[b] = max(biggest[b], int(claim_dev.sum()))
    assert np.array_equal(st["labels"], np.asarray(dev["labels"]).reshape(B, -1)), (what, "labels are not the replayed claims")
    assert np.array_equal(st["count"], np.asarray(dev["count"])), (what, st["count"], dev["count"])
    assert (mism <= 2).all(), (what, "iterations whose point is not the oracle's arg-max", mism.tolist())
    assert (biggest >= 16).all(), (what, "largest claim per image", biggest.tolist())
    out = dict(e_merge=e_merge, e_pred=e_pred, gap=worst_gap, excused=worst_excused, mism=mism.tolist(),
               biggest=biggest.tolist(), iters=len(dev["s_t"]))
    print("SEGLOCK %s: iters %d  merge err %.2e  pred err %.2e (tol %.0e)  worst point gap %.2e  excused share %.4f  "
          "point != oracle arg-max %s  largest claim %s" % (what, out["iters"], e_merge, e_pred, tol, worst_gap,
                                                          worst_excused, out["mism"], out["biggest"]))
    return out


# (size, seed of synth_batch(2, size, size, seed), iterations) of the lockstep tests: the CPU test checks that the oracle
# alone (float32 against float64) stays within every bound and condition for each, the GPU test runs the HIP path on them
LOCKSTEP_CASES = [(64, 0, 12), (64, 1, 12), (256, 0, 8)]


def lockstep_inputs(size, seed):
    """(state dict, x, GT foreground bool [B,H,W]) of a lockstep case."""
    x, sem, _, _ = R.synth_batch(2, size, size, seed=seed)
    return R.synth_state_dict(), x, sem[:, 1].numpy() > 0
