"""Ground-truth-free instance inference on the GPU: isa_seg_begin / isa_seg_claim, ReSeg.segment,
Model.predict_instances and pred_list.py --instances.

1. The kernels against the numpy restatement of the procedure (tests/segment_np.py), integer equality of labels, count,
   s_t, active and the "any image active" word after every step; outputs sit inside 0xFF / -7 padded buffers whose
   padding must stay bit-unchanged.
2. segment() with the GT foreground and the GT path's points decodes what forward() decodes: every it%d.L%d.pred
   bit-identical (same kernels, same inputs; eval mode accumulates no statistics).  This is also the test that the
   once-per-call cross branches equal the per-iteration ones.
3. The whole procedure in lockstep with the float64 oracle (tests/segment_oracle.py states the bounds).
4. Invariants of the result, fp32 and bf16 storage.
5. pred_list.py --instances writes what evaluate.py reads.

Measured on MI355X: in the docstrings of the tests (their SEGLOCK / SEGINV lines); the file runs in about 35 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import reseg_ref as R           # noqa: E402
import segment_np as S          # noqa: E402
import segment_oracle as O      # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

NAN, INF = float("nan"), float("inf")
PAD = 64                        # elements of padding on either side of every output (keeps 16-byte alignment)
SEG_PART = 64 * 2               # ISA_ROW_CHUNKS * 2 floats of chunk candidates per row
EINVAL, EALIGN = -1, -2
DTYPES = [torch.float32, torch.bfloat16]


def _lib():
    L = _gpu()[0]
    return L, L.lib()


class Padded:
    """`numel` elements between two runs of PAD sentinel elements."""

    def __init__(self, numel, dtype, fill):
        self.numel, self.fill = numel, fill
        self.buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + numel]

    def pads_unchanged(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == self.fill).all()) and bool((b[PAD + self.numel:] == self.fill).all())


class KernelState:
    """Device buffers of the two entry points, and the step-by-step comparison with the restatement."""

    def __init__(self, sem, merge):
        self.L, self.lib = _lib()
        self.sem_np, self.merge_np = np.asarray(sem, np.float32), np.asarray(merge, np.float32)
        self.B, self.Lp = self.sem_np.shape
        self.sem, self.merge = torch.from_numpy(self.sem_np).cuda(), torch.from_numpy(self.merge_np).cuda()
        B = self.B
        self.labels = Padded(B * self.Lp, torch.uint8, 0xFF)
        self.count, self.s_t, self.active = (Padded(B, torch.int32, -7) for _ in range(3))
        self.any = Padded(1, torch.int32, -7)
        self.part = torch.full((B * SEG_PART + PAD,), NAN, device="cuda")
        self.ref = None

    def ptrs(self):
        P = self.L.ptr
        return P(self.labels.view), P(self.count.view), P(self.s_t.view), P(self.active.view), P(self.any.view)

    def begin(self):
        L = self.L
        lab, cnt, st, act, anyp = self.ptrs()
        L.check(self.lib.isa_seg_begin(L.ptr(self.sem), L.ptr(self.merge), self.B, self.Lp, lab, cnt, st, act, anyp,
                                       L.ptr(self.part), L.stream_ptr()), "isa_seg_begin")
        self.ref = S.seg_begin(self.sem_np, self.merge_np)
        self.compare("begin")

    def claim(self, pred, dtype, ld, s_inject=None, what="claim"):
        """pred: float32 numpy [B,Lp,2]; stored as `dtype` with pixel stride ld (the padding channels hold NaN)."""
        L = self.L
        B, Lp = self.B, self.Lp
        store = torch.full((B, Lp, ld), NAN, dtype=dtype, device="cuda")
        pt = torch.from_numpy(np.asarray(pred, np.float32)).to(dtype)
        store[:, :, :2] = pt.cuda()
        h = 1 if Lp % 16 else 16
        desc = L.IsaTensor(store.data_ptr(), B, h, Lp // h, 2, ld, L.dtype_code(dtype), 1)
        lab, cnt, st, act, anyp = self.ptrs()
        s_in = st
        if s_inject is not None:
            s_dev = torch.tensor(s_inject, dtype=torch.int32, device="cuda")
            s_in = L.ptr(s_dev)
        L.check(self.lib.isa_seg_claim(desc, L.ptr(self.sem), L.ptr(self.merge), s_in, lab, cnt, act, st, anyp,
                                       L.ptr(self.part), L.stream_ptr()), "isa_seg_claim")
        S.seg_claim(self.ref, pt.float().numpy(), self.sem_np, self.merge_np,
                    None if s_inject is None else np.asarray(s_inject))
        self.compare(what)

    def snapshot(self):
        torch.cuda.synchronize()
        return dict(labels=self.labels.view.cpu().numpy().reshape(self.B, self.Lp).copy(),
                    count=self.count.view.cpu().numpy().copy(), s_t=self.s_t.view.cpu().numpy().copy(),
                    active=self.active.view.cpu().numpy().copy(), any=int(self.any.view.cpu()[0]))

    def compare(self, what):
        got = self.snapshot()
        for k in ("count", "active", "s_t", "labels"):
            bad = np.argwhere(got[k] != self.ref[k])
            assert bad.size == 0, (what, k, bad[:4].tolist(), got[k][tuple(bad[0])], self.ref[k][tuple(bad[0])])
        assert got["any"] == self.ref["any"], (what, "any", got["any"], self.ref["any"])
        for nm in ("labels", "count", "s_t", "active", "any"):
            assert getattr(self, nm).pads_unchanged(), (what, nm, "padding written")
        assert bool(torch.isnan(self.part[self.B * SEG_PART:]).all()), (what, "part padding written")


def random_case(B, Lp, seed, fg_share=0.5):
    """Foreground in runs, scores on a grid of 8 values (ties everywhere), logits with a few NaN."""
    rs = np.random.RandomState(seed)
    sem = (rs.rand(B, Lp // 4) < fg_share).repeat(4, axis=1).astype(np.float32)
    sem[:, ::7] = (rs.rand(B, len(range(0, Lp, 7))) < fg_share)
    merge = (rs.randint(0, 8, (B, Lp)) / 8.0).astype(np.float32)

    def pred():
        p = rs.standard_normal((B, Lp, 2)).astype(np.float32)
        p[:, :, 1] -= 1.5                                       # about one pixel in seven is claimed per step
        p[rs.rand(B, Lp) < 0.01, 0] = NAN
        p[rs.rand(B, Lp) < 0.01, 1] = NAN
        return p
    return sem, merge, pred


# ---- 1. the kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lp", [16 * 16, 64 * 64, 256 * 256, 48 * 80])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_kernels_against_the_restatement(B, Lp, dtype):
    """Four claim steps on random inputs, ld = 2 (16-byte loads of pred) and ld = 8 (the decoder's own stride) in turn."""
    sem, merge, pred = random_case(B, Lp, seed=B * 1000 + Lp % 997)
    sem[B - 1, : Lp // 2] = 0                                     # a long run of background
    ks = KernelState(sem, merge)
    ks.begin()
    for step in range(4):
        ks.claim(pred(), dtype, 2 if step % 2 == 0 else 8, what="step %d" % step)
    assert ks.ref["count"].max() == 4


def test_ties_first_index_wins_also_across_chunks():
    """Lp = 65536 is 16 chunks of 4096 pixels.  Equal maxima at 5000 and 60000 (chunks 1 and 14): 5000; all scores
    equal: the first foreground pixel; a larger value in a later chunk still wins; after the winner is claimed the
    other maximum is next."""
    Lp = 65536
    sem = np.ones((3, Lp), np.float32)
    sem[1, :777] = 0
    merge = np.zeros((3, Lp), np.float32)
    merge[0, 5000] = merge[0, 60000] = 2.0
    merge[1, :] = 0.5
    merge[2, 5000], merge[2, 60000] = 2.0, 3.0
    ks = KernelState(sem, merge)
    ks.begin()
    assert ks.ref["s_t"].tolist() == [5000, 777, 60000]
    nothing = np.stack([np.ones((3, Lp), np.float32), np.zeros((3, Lp), np.float32)], 2)      # l1 < l0: point only
    ks.claim(nothing, torch.float32, 8)
    assert ks.ref["s_t"].tolist() == [60000, 778, 5000]
    ks.claim(nothing, torch.bfloat16, 2)
    assert ks.ref["count"].tolist() == [2, 2, 2]


def test_nan_and_inf_scores_nan_logits():
    """NaN never wins, -inf loses to any number; rows of only NaN / -inf give their first remaining pixel; +inf wins;
    a NaN logit claims nothing (both orders), equal logits claim nothing."""
    Lp = 64 * 64
    rs = np.random.RandomState(5)
    sem = np.ones((5, Lp), np.float32)
    sem[:, :9] = 0
    merge = rs.rand(5, Lp).astype(np.float32)
    merge[0, 100] = NAN
    merge[0, 3000] = 7.0
    merge[1, :] = NAN
    merge[2, :] = -INF
    merge[3, ::2], merge[3, 1::2] = NAN, -INF
    merge[4, 2000] = INF
    ks = KernelState(sem, merge)
    ks.begin()
    assert ks.ref["s_t"].tolist() == [3000, 9, 9, 9, 2000]
    pred = np.zeros((5, Lp, 2), np.float32)
    pred[:, 0::4, 0] = NAN
    pred[:, 0::4, 1] = 1.0
    pred[:, 1::4, 1] = NAN
    pred[:, 2::4, :] = 0.25
    pred[:, 3::4, 1] = 1.0                                        # the only claimed pixels, besides the points
    for dtype, ld in ((torch.float32, 8), (torch.bfloat16, 8), (torch.float32, 2)):
        ks.claim(pred, dtype, ld)
        pred[:, 3::4, 1] = 0.0
    lab = ks.ref["labels"]
    assert (lab[:, 3::4][:, 3:] == 1).all() and lab[1, 9] == 1 and lab[1, 10] == 2 and lab[1, 12] == 3


def test_empty_inactive_and_label_limit():
    """An image without foreground from the start; an image that goes inactive while the others go on (it keeps its
    count and labels, its point is 0); count 254 -> 255 gives label 255, after which the image claims nothing."""
    Lp = 48 * 80
    sem, merge, pred = random_case(4, Lp, seed=9)
    sem[0, :] = 0
    sem[1, :] = 0
    sem[1, 40:52] = 1
    ks = KernelState(sem, merge)
    ks.begin()
    assert ks.ref["active"].tolist() == [0, 1, 1, 1] and ks.ref["s_t"][0] == 0
    p = pred()
    p[1, :, 0], p[1, :, 1] = 0.0, 1.0                             # image 1 is explained by its first instance
    ks.claim(p, torch.float32, 8)
    assert ks.ref["active"].tolist() == [0, 0, 1, 1] and ks.ref["count"].tolist() == [0, 1, 1, 1]
    ks.claim(pred(), torch.bfloat16, 8)
    assert ks.ref["count"].tolist() == [0, 1, 2, 2] and ks.ref["any"] == 1
    ks.count.view[2] = 254                                        # jump ahead: the next instance of image 2 is number 255
    ks.ref["count"][2] = 254
    ks.claim(pred(), torch.float32, 2)
    assert ks.ref["count"].tolist() == [0, 1, 255, 3] and (ks.ref["labels"][2] == 255).any()
    before = ks.ref["labels"][2].copy()
    ks.claim(pred(), torch.float32, 8)
    assert ks.ref["count"].tolist() == [0, 1, 255, 4] and np.array_equal(ks.ref["labels"][2], before)
    assert ks.ref["active"][2] == 1


def test_injected_points():
    """s_t as an input of its own (injected points): a point outside the remaining set claims nothing by itself."""
    Lp = 64 * 64
    sem, merge, pred = random_case(3, Lp, seed=21)
    ks = KernelState(sem, merge)
    ks.begin()
    bg = int(np.flatnonzero(sem[0] < 0.5)[0])
    fgp = [int(np.flatnonzero(sem[b] > 0.5)[5]) for b in range(3)]
    nothing = np.stack([np.ones((3, Lp), np.float32), np.zeros((3, Lp), np.float32)], 2)
    ks.claim(nothing, torch.float32, 8, s_inject=[bg, fgp[1], fgp[2]])
    assert (ks.ref["labels"] != 0).sum(1).tolist() == [0, 1, 1] and ks.ref["count"].tolist() == [1, 1, 1]
    ks.claim(pred(), torch.bfloat16, 2, s_inject=fgp)


def test_fold_is_deterministic():
    """Ten repeats of 16 x 65536 with ties in every chunk: identical bits of every output."""
    sem, merge, pred = random_case(16, 65536, seed=77)
    preds = [pred() for _ in range(3)]
    first = None
    for rep in range(10):
        ks = KernelState(sem, merge)
        ks.begin()
        for i, p in enumerate(preds):
            ks.claim(p, torch.float32, 8 if i != 1 else 2)
        snap = ks.snapshot()
        if first is None:
            first = snap
        for k in ("labels", "count", "s_t", "active"):
            assert np.array_equal(first[k], snap[k]), (rep, k)


def test_refused_calls_write_nothing():
    L, lib = _lib()
    sem, merge, pred = random_case(2, 1024, seed=3)
    ks = KernelState(sem, merge)
    lab, cnt, st, act, anyp = ks.ptrs()
    args = (L.ptr(ks.sem), L.ptr(ks.merge))
    assert lib.isa_seg_begin(*args, 2, 1022, lab, cnt, st, act, anyp, L.ptr(ks.part), L.stream_ptr()) == EINVAL
    assert lib.isa_seg_begin(*args, 0, 1024, lab, cnt, st, act, anyp, L.ptr(ks.part), L.stream_ptr()) == EINVAL
    assert lib.isa_seg_begin(*args, 2, 1024, lab, None, st, act, anyp, L.ptr(ks.part), L.stream_ptr()) == EINVAL
    odd = L.ptr(ks.labels.buf[PAD + 1:])
    assert lib.isa_seg_begin(*args, 2, 1020, odd, cnt, st, act, anyp, L.ptr(ks.part), L.stream_ptr()) == EALIGN
    store = torch.zeros(2, 1024, 8, device="cuda")
    bad_c = L.IsaTensor(store.data_ptr(), 2, 32, 32, 3, 8, L.F32, 1)
    assert lib.isa_seg_claim(bad_c, *args, st, lab, cnt, act, st, anyp, L.ptr(ks.part), L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((ks.labels.buf == 0xFF).all()) and bool((ks.count.buf == -7).all()) and bool((ks.s_t.buf == -7).all())
    assert bool(torch.isnan(ks.part).all())


# ---- the model ------------------------------------------------------------------------------------------------------
def build(dtype, sd=None):
    _gpu()
    from isa_amd.reseg import ReSeg
    m = ReSeg(2, True, dtype=dtype)
    m.load_state_dict(sd if sd is not None else R.synth_state_dict())
    m.eval()
    m.head.drop_rate = 0.0
    return m


def pred_rows(act):
    """A captured level prediction as float32 numpy [B, h*w, 2]."""
    t = act.nchw().cpu()
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, 2).numpy()


# ---- 2. the same decode as the ground-truth path ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [64, 256])
def test_same_decode_as_the_ground_truth_path(size, dtype):
    """forward(False, x, sem, ins, N) picks its points on the GT planes; segment(x, sem_map = GT foreground,
    injected_s_t = those points) must produce bit-identical it%d.L%d.pred: the decoder pass reads the backbone
    features, the pooled foreground and the point, and none of the launches in that chain accumulates in an order that
    depends on execution (no float atomics feed an output in eval mode).  synth_batch is asked for T = 4 objects in
    every image; forward runs min(N) iterations, which is what is compared."""
    T = 4
    x, sem, ins, n = R.synth_batch(2, size, size, seed=3, kmin=T, kmax=T)
    m = build(dtype)
    sel = [list(range(int(k))) for k in n.view(-1)]
    cap_gt = {}
    m(False, x, sem, ins, n, selected_idx=sel, capture=cap_gt)
    torch.cuda.synchronize()
    iters = m.last_record["iters"]
    assert len(iters) == int(n.min()) >= 2
    points = [r["s_t"].clone() for r in iters]
    want = {k: v.buf.clone() for k, v in cap_gt.items() if k.endswith(".pred")}
    cap = {}
    fg = sem[:, 1].float().reshape(2, -1)
    _, _, labels, count = m.segment(x, sem_map=fg, injected_s_t=points, capture=cap)
    torch.cuda.synchronize()
    assert m.head.seg_passes == len(points) and count.tolist() == [len(points)] * 2
    for t in range(len(points)):
        assert torch.equal(cap["it%d.s_t" % t], points[t])
        for lvl in range(5):
            k = "it%d.L%d.pred" % (t, lvl)
            a, b = cap[k].buf[..., :2].contiguous(), want[k][..., :2].contiguous()
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(a.view(bits), b.view(bits)), (k, float((a.float() - b.float()).abs().max()))
    assert int((labels != 0).sum()) > 0 and bool((labels.cpu()[sem[:, 1] == 0] == 0).all())


# ---- 3. lockstep with the float64 oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("size,seed,iters", O.LOCKSTEP_CASES)
def test_lockstep_with_the_oracle(size, seed, iters):
    """fp32 storage, synth_state_dict() weights, GT foreground as sem_map, B = 2; bounds and conditions: see
    tests/segment_oracle.py.  Measured on MI355X (SEGLOCK lines), 64 x 64 seed 0 / seed 1 / 256 x 256: merge error
    6.9e-6 / 7.6e-6 / 1.0e-5, worst pred error 5.4e-5 / 4.8e-5 / 1.3e-4 (bound 1e-3), every point the float64 oracle's
    own arg-max (gap 0), excused share 0.35 / 0.36 / 0.24 % of the foreground (cap 1 %), largest claims 62 and 29, 47 and
    55, 1374 and 929 pixels; all images run to the cap."""
    sd, x, fg = O.lockstep_inputs(size, seed)
    m = build(torch.float32, sd)
    cap = {}
    fgt = torch.from_numpy(fg.reshape(2, -1).astype(np.float32))
    _, _, labels, count = m.segment(x, max_objects=iters, sem_map=fgt, capture=cap)
    torch.cuda.synchronize()
    T = m.head.seg_passes
    assert T == iters, "the case runs to the cap with untrained weights"
    dev = dict(merge=cap["merge"].view(2, -1).cpu().numpy(), s_t=[cap["it%d.s_t" % t].cpu().numpy() for t in range(T)],
               pred=[pred_rows(cap["it%d.L4.pred" % t]) for t in range(T)], labels=labels.cpu().numpy().reshape(2, -1),
               count=count.cpu().numpy())
    torch.set_num_threads(min(16, torch.get_num_threads()))
    O.lockstep(dev, O.Oracle(sd, x, fg, torch.float64), fg, "HIP fp32 vs f64 oracle %dx%d seed %d" % (size, size, seed))


# ---- 4. invariants --------------------------------------------------------------------------------------------------
def best_match_iou(a, b):
    """Mean over the instances of label map a of their best IoU with an instance of b."""
    out = []
    for k in range(1, int(a.max()) + 1):
        ma = a == k
        best = 0.0
        for j in np.unique(b[ma]):
            if j:
                mb = b == j
                best = max(best, float((ma & mb).sum()) / float((ma | mb).sum()))
        out.append(best)
    return float(np.mean(out)) if out else 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_invariants(dtype):
    """Predicted foreground, B = 5, image 3 made all background through sem_map.  The bf16-against-fp32 agreement of
    the label maps (best-match IoU, SEGINV line) is printed, not gated: the loop turns one flipped point into another
    partition.  Measured on MI355X: every image with foreground runs to 32 instances in both precisions (untrained
    weights: most claims after the first are a few pixels), alone == in batch also in bf16, best-match IoU of the bf16
    labels against the fp32 labels 0.42 - 0.58 per image."""
    B, size, EMPTY = 5, 64, 3
    x, _, _, _ = R.synth_batch(B, size, size, seed=11)
    m = build(dtype)
    _, arg = m.segment(x, max_objects=1)[:2]
    fg = (arg[:, 0] > 0.5).float().reshape(B, -1).clone()
    fg[EMPTY] = 0
    fg_np = fg.cpu().numpy() > 0.5
    assert all(fg_np[b].sum() >= 32 for b in range(B) if b != EMPTY), fg_np.sum(1)

    def run(k, xs=x, fgs=fg, cap=None):
        out = m.segment(xs, max_objects=k, sem_map=fgs, capture=cap)
        torch.cuda.synchronize()
        return out[2].cpu().numpy().reshape(len(xs), -1), out[3].cpu().numpy()

    E = m.engine
    arena_bytes = lambda: (len(E.arena.slots), E.arena.bytes(), E.arena.stats.numel())
    lab2, n2 = run(2)
    small = arena_bytes()
    cap = {}
    lab, n = run(32, cap=cap)
    assert arena_bytes() == small, "the arena must not grow with max_objects"
    passes = m.head.seg_passes
    assert n[EMPTY] == 0 and not lab[EMPTY].any()
    assert (n <= 32).all() and n.max() >= 3
    for b in range(B):
        assert lab[b].max() == n[b] and not lab[b][~fg_np[b]].any()
        points = [int(cap["it%d.s_t" % t][b]) for t in range(n[b])]
        assert len(set(points)) == len(points), "points pairwise distinct"
        for k in range(1, n[b] + 1):
            assert (lab[b] == k).any() and lab[b][points[k - 1]] == k, (b, k)
        if n[b] < 32:
            assert not (fg_np[b] & (lab[b] == 0)).any(), "an image stops early only when it is explained"
    # the cap: a prefix of the same sequence of instances
    for k, (lk, nk) in ((2, (lab2, n2)), (1, run(1)), (3, run(3))):
        assert np.array_equal(nk, np.minimum(n, k)), (k, nk, n)
        assert np.array_equal(lk, np.where(lab <= k, lab, 0)), k
    # two calls in a row
    lab_b, n_b = run(32)
    assert np.array_equal(lab_b, lab) and np.array_equal(n_b, n)
    # an image alone and inside the batch
    same = []
    for b in (0, EMPTY, 4):
        la, na = run(32, x[b:b + 1], fg[b:b + 1])
        same.append(bool(np.array_equal(la[0], lab[b]) and na[0] == n[b]))
    if dtype == torch.float32:
        assert all(same), same
    print("SEGINV %s: n_objects %s, passes %d, alone == in batch %s" % (dtype, n.tolist(), passes, same))
    if dtype == torch.bfloat16:
        m32 = build(torch.float32)
        out = m32.segment(x, max_objects=32, sem_map=fg)
        l32 = out[2].cpu().numpy().reshape(B, -1)
        print("SEGINV bf16 vs fp32 labels: best-match IoU per image %s, n_objects fp32 %s"
              % (["%.3f" % best_match_iou(l32[b], lab[b]) for b in range(B)], out[3].tolist()))
    m.train()
    with pytest.raises(AssertionError):
        m.segment(x)
    m.eval()
    with pytest.raises(ValueError):
        m.segment(x, max_objects=256)
    with pytest.raises(RuntimeError):                            # forward keeps refusing GT-free instance input
        m(False, x)


def test_predict_instances():
    _gpu()
    from isa_amd.model import Model
    x, _, _, _ = R.synth_batch(2, 64, 64, seed=2)
    model = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=True)
    prob, labels, n = model.predict_instances(x)
    assert tuple(prob.shape) == (2, 64, 64) and labels.dtype == torch.uint8 and tuple(labels.shape) == (2, 64, 64)
    assert n.dtype == torch.int32 and tuple(n.shape) == (2,) and int(n.max()) <= 5
    assert not prob.is_cuda and not labels.is_cuda and not n.is_cuda
    assert bool((labels[prob < 0.499] == 0).all()), "labels lie inside the predicted foreground"
    assert all(int(labels[b].max()) == int(n[b]) for b in range(2))
    sem_only = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=False)
    with pytest.raises(RuntimeError):
        sem_only.predict_instances(x)
    with pytest.raises(RuntimeError):
        model.predict(x)


# ---- 5. end to end --------------------------------------------------------------------------------------------------
def test_pred_list_instances_and_evaluate(tmp_path):
    """pred_list.py --instances writes five files per image in the formats evaluate.py reads: a data root whose label
    images are copies of the predictions scores SBD = 1 and |DiC| = 0 on every image.  Without the flag the script
    writes the two files it always wrote."""
    from PIL import Image
    _gpu()
    out, plain = str(tmp_path / "ins"), str(tmp_path / "plain")
    script = os.path.join(ROOT, "pred_list.py")
    for args in (["--instances", "--output", out], ["--output", plain]):
        r = subprocess.run([sys.executable, script, "--synthetic", "6", "--batch", "4"] + args,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ["synthetic_%04d" % i for i in range(6)] and sorted(os.listdir(plain)) == names
    root = tmp_path / "data"
    img_dir = root / "raw/CVPPP/CVPPP2017_LSC_training/training/A1"
    os.makedirs(img_dir)
    os.makedirs(root / "metadata/CVPPP")
    rows = []
    for i, name in enumerate(names):
        d = os.path.join(out, name)
        assert sorted(os.listdir(d)) == sorted(name + s for s in ("-fg_mask.png", "-ins_mask.png", "-ins_mask_color.png",
                                                                  "-n_objects.npy", ".png"))
        assert sorted(os.listdir(os.path.join(plain, name))) == sorted([name + ".png", name + "-fg_mask.png"])
        src = Image.open(os.path.join(d, name + ".png"))
        ins_img = Image.open(os.path.join(d, name + "-ins_mask.png"))
        assert ins_img.mode == "L" and ins_img.size == src.size == (330, 300 + 7 * (i % 5))
        ins = np.array(ins_img)
        fgm = np.array(Image.open(os.path.join(d, name + "-fg_mask.png")))
        n = np.load(os.path.join(d, name + "-n_objects.npy"))
        assert ins.dtype == np.uint8 and int(n) == int(ins.max()) and 1 <= int(n) <= 32
        assert set(np.unique(ins)) <= set(range(int(n) + 1)) and not ins[fgm == 0].any()
        col = Image.open(os.path.join(d, name + "-ins_mask_color.png"))
        assert col.mode == "RGB" and col.size == src.size and not np.array(col)[ins == 0].any()
        assert np.array_equal(fgm, np.array(Image.open(os.path.join(plain, name, name + "-fg_mask.png"))))
        Image.fromarray(ins).save(img_dir / (name + "_label.png"))
        Image.fromarray((fgm == 255).astype(np.uint8)).save(img_dir / (name + "_fg.png"))
        rows.append("%s,%d" % (name, int(n)))
    (root / "metadata/CVPPP/validation_image_paths.txt").write_text("".join("x/%s.png\n" % nm for nm in names))
    (root / "metadata/CVPPP/number_of_instances.txt").write_text("\n".join(rows) + "\n")
    sys.path.insert(0, ROOT)
    from evaluate import evaluate_cvppp
    sbds, dics, fg_dices, scored = evaluate_cvppp(out, str(root))
    assert scored == names
    assert sbds == [1.0] * 6 and [int(v) for v in dics] == [0] * 6 and fg_dices == [1.0] * 6


def test_pred_instances_single_image(tmp_path):
    """pred.py --instances: the three instance files next to the palette foreground mask, at the original size."""
    from PIL import Image
    _gpu()
    out = str(tmp_path / "one")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred.py"), "--synthetic", "--instances", "--max-objects", "5",
                        "--output", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == sorted("synthetic" + s for s in ("-fg_mask.png", "-ins_mask.png",
                                                                      "-ins_mask_color.png", "-n_objects.npy"))
    ins = np.array(Image.open(os.path.join(out, "synthetic-ins_mask.png")))
    fgm = np.array(Image.open(os.path.join(out, "synthetic-fg_mask.png")))            # palette indices {0, 255}
    n = int(np.load(os.path.join(out, "synthetic-n_objects.npy")))
    assert ins.shape == (530, 500) and ins.dtype == np.uint8 and n == int(ins.max()) and 1 <= n <= 5
    assert not ins[fgm == 0].any()
