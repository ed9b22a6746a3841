"""CPU checks of ground-truth-free instance inference: the numpy restatement of the procedure (tests/segment_np.py) on
hand-made cases with known answers, that those cases tell the likely wrong kernels apart, and that the oracle alone
(float32 blocks against float64 blocks of oracle/reseg_ref.py) stays within every bound and condition of the lockstep
test for each seed and size the GPU test uses - a badly chosen seed shows up here and not as a GPU failure."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import segment_np as S          # noqa: E402

NAN, INF = float("nan"), float("inf")


def logits(fg_mask):
    """[L,2] logits that call exactly the pixels of fg_mask foreground."""
    m = np.asarray(fg_mask, bool).reshape(-1)
    return np.stack([np.where(m, 0.0, 1.0), np.where(m, 1.0, 0.0)], 1)


# ---- the hand-made cases: (fg [B,L], merge [B,L], decode, max_objects) -> expected (labels, count) ---------------------
def case_two_squares():
    """8 x 8, two 3 x 3 squares; the decoder returns the square that holds the point."""
    a, b = np.zeros((8, 8), bool), np.zeros((8, 8), bool)
    a[1:4, 1:4] = True
    b[4:7, 4:7] = True
    fg = (a | b).reshape(1, -1).astype(np.float32)
    merge = fg.copy()
    merge[0, 2 * 8 + 2], merge[0, 5 * 8 + 5] = 4.0, 5.0                  # the second square's peak is higher: found first
    decode = lambda s: np.stack([logits(a if a.reshape(-1)[s[0]] else b)])
    want = (np.where(b, 1, 0) + np.where(a, 2, 0)).reshape(1, -1).astype(np.uint8)
    return fg, merge, decode, 32, want, np.array([2], np.int32)


def _rows_decode(s):
    m = np.zeros((4, 4), bool)
    m[s[0] // 4] = True
    return np.stack([logits(m)])


def case_tie():
    """4 x 4, every score equal: the first index wins, the decoder returns the row of the point -> rows 1, 2, 3, 4."""
    fg, merge = np.ones((1, 16), np.float32), np.full((1, 16), 0.25, np.float32)
    want = np.repeat(np.arange(1, 5), 4).reshape(1, -1).astype(np.uint8)
    return fg, merge, _rows_decode, 32, want, np.array([4], np.int32)


def case_cap():
    """The tie case stopped at max_objects = 2: the foreground left over keeps label 0."""
    fg, merge, decode, _, want, _ = case_tie()
    want = want.copy()
    want[want > 2] = 0
    return fg, merge, decode, 2, want, np.array([2], np.int32)


def case_forced_point():
    """The decoder says background everywhere - with equal logits on one pixel, which `>` must not take: every
    iteration claims its point and nothing else, in the order of the scores."""
    fg = np.zeros((1, 16), np.float32)
    fg[0, [3, 9, 12]] = 1
    merge = np.zeros((1, 16), np.float32)
    merge[0, 3], merge[0, 9], merge[0, 12] = 1.0, 3.0, 2.0
    lg = logits(np.zeros(16, bool))
    lg[12] = (0.5, 0.5)

    def decode(s):
        return np.stack([lg])
    want = np.zeros((1, 16), np.uint8)
    want[0, 9], want[0, 12], want[0, 3] = 1, 2, 3
    return fg, merge, decode, 32, want, np.array([3], np.int32)


def case_no_overwrite():
    """Two squares, but the second pass predicts the whole foreground: the first instance keeps its pixels."""
    fg, merge, _, _, want, count = case_two_squares()
    first = want[0] == 1

    def decode(s):
        return np.stack([logits(first if first[s[0]] else fg[0] > 0)])
    return fg, merge, decode, 32, want, count


def case_inactive():
    """Two images; the decoder returns the row of the point.  Image 0 has one row of foreground and goes inactive
    after the first pass while image 1 (three rows) goes on: image 0 keeps count 1 and its labels; image 2 is empty
    from the start."""
    fg = np.zeros((3, 16), np.float32)
    fg[0, 4:8] = 1
    fg[1, 0:12] = 1
    merge = np.tile(np.arange(16, 0, -1, dtype=np.float32), (3, 1))

    def decode(s):
        return np.concatenate([_rows_decode([v]) for v in s])
    want = np.zeros((3, 16), np.uint8)
    want[0, 4:8] = 1
    want[1, 0:12] = np.repeat([1, 2, 3], 4)
    return fg, merge, decode, 32, want, np.array([1, 3, 0], np.int32)


CASES = dict(two_squares=case_two_squares, tie=case_tie, cap=case_cap, forced_point=case_forced_point,
             no_overwrite=case_no_overwrite, inactive=case_inactive)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_known_answers(name):
    fg, merge, decode, cap, want, count = CASES[name]()
    labels, got_count, trace = S.segment_loop(fg, merge, decode, cap)
    assert np.array_equal(labels, want), (name, labels.reshape(len(fg), -1))
    assert np.array_equal(got_count, count), (name, got_count)
    assert len(trace) == int(count.max()), "the loop stops when no image is active, or at the cap"
    for t in trace:                                            # the point of an active image is a remaining pixel
        for b in range(len(fg)):
            assert not t["active"][b] or fg[b, t["s_t"][b]] > 0.5
            assert t["active"][b] or t["s_t"][b] == 0


# which hand-made case exposes which mistake
CAUGHT_BY = dict(last_max="tie", no_forced_point="forced_point", ge="forced_point", overwrite="no_overwrite",
                 relabel_inactive="inactive")


@pytest.mark.parametrize("flaw", S.FLAWS)
def test_cases_tell_wrong_kernels_apart(flaw):
    fg, merge, decode, cap, want, count = CASES[CAUGHT_BY[flaw]]()
    labels, got_count, _ = S.segment_loop(fg, merge, decode, cap, flaws=(flaw,))
    assert not (np.array_equal(labels, want) and np.array_equal(got_count, count)), flaw


def test_argmax_rules():
    """First maximum; NaN never wins; -inf and NaN only: the first remaining pixel; empty mask: none."""
    f = S.masked_first_argmax
    m = np.array([0, 1, 1, 1, 1, 0], bool)
    assert f(np.array([9.0, 1.0, 3.0, 3.0, 2.0, 9.0]), m) == 2
    assert f(np.array([9.0, NAN, 3.0, INF, NAN, 9.0]), m) == 3
    assert f(np.array([9.0, NAN, -INF, NAN, -INF, 9.0]), m) == 1
    assert f(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), np.zeros(6, bool)) == -1
    assert f(np.array([0.0, -0.0, 0.0, -1.0, -1.0, 0.0]), m) == 1            # -0.0 == 0.0: a tie


def test_nan_logits_and_label_limit():
    """`>` on a NaN logit is false; an image that holds 255 instances claims nothing more (labels are uint8)."""
    fg, merge = np.ones((1, 4), np.float32), np.array([[4.0, 3.0, 2.0, 1.0]], np.float32)
    pred = np.array([[[0.0, 1.0], [NAN, 1.0], [0.0, NAN], [1.0, 0.0]]])
    st = S.seg_begin(fg, merge)
    S.seg_claim(st, pred, fg, merge)
    assert st["labels"].tolist() == [[1, 0, 0, 0]] and st["count"].tolist() == [1] and st["s_t"].tolist() == [1]
    st["count"][0] = 254
    S.seg_claim(st, pred, fg, merge)                           # claims its point (pixel 1) as instance 255
    assert st["labels"].tolist() == [[1, 255, 0, 0]] and st["count"].tolist() == [255]
    S.seg_claim(st, pred, fg, merge)
    assert st["labels"].tolist() == [[1, 255, 0, 0]] and st["count"].tolist() == [255] and st["active"].tolist() == [1]


# ---- the oracle alone, for every case of the GPU lockstep test -------------------------------------------------------
def test_lockstep_cases_hold_for_the_oracle_alone():
    """float32 oracle against float64 oracle through tests/segment_oracle.lockstep for each (size, seed, iterations)
    of LOCKSTEP_CASES, with the GT foreground as sem_map.  Measured (SEGLOCK lines, float32 against float64): merge error
    5e-6 - 1e-5, pred error 9e-5 - 1e-4, no iteration whose point differs from the float64 arg-max, excused share at
    most 0.36 % of the foreground, largest claims 62 / 29, 47 / 55 and 1374 / 929 pixels."""
    import segment_oracle as O
    torch.set_num_threads(min(8, torch.get_num_threads()))
    for size, seed, iters in O.LOCKSTEP_CASES:
        sd, x, fg = O.lockstep_inputs(size, seed)
        assert fg.reshape(2, -1).sum(1).min() >= 100
        ref = O.Oracle(sd, x, fg, torch.float64)
        dev = O.run_loop(O.Oracle(sd, x, fg, torch.float32), fg, iters)
        assert len(dev["s_t"]) == iters
        O.lockstep(dev, ref, fg, "oracle f32 vs f64 %dx%d seed %d" % (size, size, seed))
