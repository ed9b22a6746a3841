"""GPU: the pixel-weighted K-class criterion (isa_sem_loss_k_sums_pw, isa_sem_loss_k_grad_pw) and the border term of the
training step built on it (Trainer(border_weight, border_sigma), Trainer.set_border).

Op level: float64 torch autograd of (cross_entropy(reduction='none', weight=w) * m).sum() / (w[y] * m).sum() plus the
unchanged Dice, to the bounds tests/test_gpu_sem_criterion.py applies to these kernels: loss 1e-5 relative, gradient 1e-5
relative L2 for fp32 logits and 8e-3 for bf16 (the restatement sees the same bf16-rounded logits).
Step level: the CE the step reports against the float64 restatement on the captured logits, the targets and the weight map
of tests/distance_np.py, within 1e-4 (the bound of the existing step-level test)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import distance_np as dn                                                        # noqa: E402
from test_gpu_sem_criterion import _cfg, _desc, _inputs, _lib, _rel_l2, _run     # noqa: E402


def _run_pw(L, buf, lab, cfg, pixw, B, K, H, W, dtype):
    lib = L.lib()
    x = _desc(L, buf, B, H, W, K, dtype)
    sums = torch.zeros(3 * B * K + 2, device="cuda")
    coef = torch.full((3 * B * K + 1,), float("nan"), device="cuda")
    scal = torch.full((2,), float("nan"), device="cuda")
    dx = torch.full_like(buf, float("nan"))
    d = _desc(L, dx, B, H, W, K, dtype)
    s = L.stream_ptr()
    L.check(lib.isa_sem_loss_k_sums_pw(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(pixw), L.ptr(sums), s), "sums_pw")
    L.check(lib.isa_sem_loss_k_assemble(L.ptr(sums), L.ptr(cfg), B, K, L.ptr(coef), L.ptr(scal), s), "assemble")
    L.check(lib.isa_sem_loss_k_grad_pw(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(coef), L.ptr(pixw), C.byref(d), 0, s), "grad_pw")
    torch.cuda.synchronize()
    return scal.cpu().double().numpy(), dx, coef


def _torch_pw(seen, lab_np, crit, weights, bg, pixw):
    """(ce, dice, d logits) in float64 autograd; ce / dice None for a term the criterion lacks."""
    logits = torch.from_numpy(seen).clone().requires_grad_(True)                  # [B,K,H,W] float64
    B, K = logits.shape[:2]
    y = torch.from_numpy(lab_np)
    w = torch.ones(K, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    m = torch.from_numpy(pixw).double()
    ce = dice = None
    cost = 0
    if crit in ("CE", "Multi"):
        nll = torch.nn.functional.cross_entropy(logits, y, weight=w, reduction="none")      # w[y] * nll per pixel
        ce = (nll * m).sum() / (w[y] * m).sum()
        cost = cost + ce
    if crit in ("Dice", "Multi"):
        p, g = torch.softmax(logits, 1), torch.nn.functional.one_hot(y, K).permute(0, 3, 1, 2).double()
        D = (2 * (p * g).sum((2, 3)) + 1) / (p.sum((2, 3)) + g.sum((2, 3)) + 1)
        Cs = list(range(0 if bg else 1, K))
        wn = len(Cs) * w[Cs] / w[Cs].sum()
        dice = (1 - (wn[None] * D[:, Cs]).mean(1)).mean()
        cost = cost + dice
    cost.backward()
    f = lambda v: None if v is None else float(v.detach())
    return f(ce), f(dice), logits.grad.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [2, 5, 12, 21, 32])          # every class width of the kernels: 8, 16, 24, 32
def test_pixel_weighted_kernels_match_float64_autograd(K, dtype):
    L = _lib()
    gbound = 1e-5 if dtype == torch.float32 else 8e-3
    B = 2
    worst = 0.0
    for H, W in ((8, 12), (72, 136)):       # 96 pixels: fewer than one workgroup of 256; 9792: no multiple of 256
        buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=K * 10 + H)
        rs = np.random.RandomState(K + H)
        pixw_np = rs.uniform(0.2, 11.0, (B, H, W)).astype(np.float32)               # random, positive
        pixw = torch.from_numpy(pixw_np).cuda()
        for crit in ("CE", "Dice", "Multi"):
            for weights in (None, list(rs.uniform(0.2, 2.0, K))):
                for bg in (False, True):
                    cfg = _cfg(crit, weights, bg, K)
                    scal, dx, _ = _run_pw(L, buf, lab, cfg, pixw, B, K, H, W, dtype)
                    ce, dice, ref_g = _torch_pw(seen, lab_np, crit, weights, bg, pixw_np)
                    tag = (K, H, crit, weights is not None, bg)
                    for got, ref in ((scal[0], ce), (scal[1], dice)):
                        if ref is None:
                            assert got == 0.0, tag
                        else:
                            assert abs(got - ref) <= 1e-5 * max(abs(ref), 1e-3), (tag, got, ref)
                    got_g = dx[..., :K].double().permute(0, 3, 1, 2).cpu().numpy()
                    e = _rel_l2(got_g, ref_g)
                    worst = max(worst, e)
                    assert e <= gbound, (tag, e)
                    assert torch.isnan(dx[..., K:]).all(), "the ld padding of d logits must stay untouched"
    print("pixel-weighted K=%d %s: worst gradient rel-L2 %.2e" % (K, dtype, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [2, 5])
def test_unit_weights_are_the_unweighted_kernels(K, dtype):
    """pixw = 1: the loss agrees with the unweighted entry to 1e-6 relative, and with the SAME coef the gradient kernel's
    output is bit-identical to isa_sem_loss_k_grad's (it has no atomics, and x * 1.0f is x)."""
    L = _lib()
    lib = L.lib()
    B = 2
    for H, W in ((8, 12), (72, 136)):
        buf, lab, _, _ = _inputs(B, K, H, W, dtype, seed=K + W)
        cfg = _cfg("Multi", [0.7, 1.9, 0.4, 1.1, 2.3][:K], True, K)
        ones = torch.ones((B, H, W), device="cuda")
        scal_pw, _, coef = _run_pw(L, buf, lab, cfg, ones, B, K, H, W, dtype)
        scal, _ = _run(L, buf, lab, cfg, B, K, H, W, dtype)
        assert np.all(np.abs(scal_pw - scal) <= 1e-6 * np.abs(scal)), (scal_pw, scal)
        x = _desc(L, buf, B, H, W, K, dtype)
        a, b = torch.full_like(buf, float("nan")), torch.full_like(buf, float("nan"))
        s = L.stream_ptr()
        L.check(lib.isa_sem_loss_k_grad(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(coef), C.byref(_desc(L, a, B, H, W, K, dtype)),
                                        0, s), "grad")
        L.check(lib.isa_sem_loss_k_grad_pw(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(coef), L.ptr(ones),
                                           C.byref(_desc(L, b, B, H, W, K, dtype)), 0, s), "grad_pw")
        torch.cuda.synchronize()
        assert torch.equal(a[..., :K].view(torch.int32 if dtype == torch.float32 else torch.int16),
                           b[..., :K].view(torch.int32 if dtype == torch.float32 else torch.int16))


# ------------------------------------------------------------------------------------------------------------ the step
def _need_model():
    _lib()
    import reseg_ref as R
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    from isa_amd.data import class_onehot
    return R, ReSeg, Trainer, class_onehot


def _two_blob_batch(R, seed):
    """x of a synthetic batch; per image two rectangles three pixels apart (planes 0 and 1), so the gap lies between two
    instances at d1 + d2 = 4: weight 1 + w0 exp(-16 / 2 sigma^2) there."""
    x, _, _, _ = R.synth_batch(2, 64, 64, seed=seed)
    ins = torch.zeros((2, 32, 64, 64), dtype=torch.int64)
    ins[0, 0, 8:50, 6:30], ins[0, 1, 12:56, 33:60] = 1, 1                        # columns 30, 31, 32 between them
    ins[1, 0, 5:28, 10:52], ins[1, 1, 31:58, 4:40] = 1, 1                        # rows 28, 29, 30 between them
    n = torch.tensor([[2], [2]], dtype=torch.int32)
    fg = ins.sum(1) > 0
    sem2 = torch.nn.functional.one_hot(fg.long(), 2).permute(0, 3, 1, 2).contiguous()
    return x, sem2, ins, n


def _label_map(ins):
    """What isa_labels_from_planes makes of the planes: 1 + the first non-zero plane, 0 where there is none."""
    ins = ins.numpy()
    return np.where(ins.any(1), ins.argmax(1) + 1, 0).astype(np.uint8)


def _ce_restatement(logits, y, pixw):
    """float64: sum m nll / sum m (no class weights)."""
    z = logits - logits.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1))
    nll = lse - np.take_along_axis(z, y[:, None], 1)[:, 0]
    return float((pixw * nll).sum() / pixw.sum())


def _models(R, ReSeg, class_onehot, which, seed):
    x, sem2, ins, n = _two_blob_batch(R, seed)
    if which == "instance":
        m = ReSeg(2, True, dtype=torch.float32)
        m.load_state_dict(R.synth_state_dict(23, True))
        m.head.drop_rate = 0.0
        sem = sem2
    else:
        from test_gpu_sem_criterion import _three_class_sd
        m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
        m.load_state_dict(_three_class_sd(R))
        sem = class_onehot(ins, 3)
    m.train()
    return m, (x, sem, ins, n)


@pytest.mark.parametrize("which", ["instance", "semantic3"])
def test_step_reports_the_border_weighted_cross_entropy(which):
    R, ReSeg, Trainer, class_onehot = _need_model()
    m, batch = _models(R, ReSeg, class_onehot, which, seed=4)
    x, sem, ins, n = batch
    tr = Trainer(m, border_weight=10.0, border_sigma=5.0)
    assert not m.net.crit.legacy and m.net.crit.border_on
    out = tr.forward_backward(*batch)
    logits = m.net.to_nchw(m._last_sem).double().cpu().numpy()
    scal = out["sem"].double().cpu().numpy()
    torch.cuda.synchronize()
    lab = _label_map(ins)
    d1, d2, _ = dn.edt2(lab)
    pixw = dn.border_weights(lab, d1, d2, 10.0, 5.0)
    assert pixw.max() > 8.0 and (pixw[lab != 0] == 1.0).all()                  # the gap: 1 + 10 exp(-16/50) = 8.26
    y = sem.argmax(1).numpy()
    ce = _ce_restatement(logits, y, pixw)
    plain = _ce_restatement(logits, y, np.ones_like(pixw))
    print("%s: CE %.6f reported, %.6f restated, %.6f unweighted" % (which, scal[0], ce, plain))
    assert abs(scal[0] - ce) <= 1e-4, (scal[0], ce)
    assert abs(scal[0] - plain) > 1e-3, (scal[0], plain)                        # the border weights matter
    assert np.isfinite(scal).all() and torch.isfinite(m.store.grad[:m.store.n_train]).all()
    # the weight map ReSeg.border_weights gives for these planes is the one the step used
    w_dev = m.border_weights(ins, 10.0, 5.0).cpu().numpy()
    assert np.abs(w_dev - pixw).max() <= 1e-6 * 11


def test_captured_step_follows_set_border_in_place():
    R, ReSeg, Trainer, class_onehot = _need_model()
    m, batch = _models(R, ReSeg, class_onehot, "semantic3", seed=5)
    tr = Trainer(m, criterion="CE", border_weight=10.0, border_sigma=5.0)
    buf = m.net.crit.border
    tr.train_step_graphed(*batch)                            # eager (configuration recorded)
    tr.train_step_graphed(*batch)                            # captured, replayed
    assert tr._graphs and list(tr._graphs.values())[0]["state"] == "ready"
    snap = m.store.flat.clone()
    tr.set_border(3.0, 2.0)                                  # in place: the graph reads this buffer
    assert m.net.crit.border.data_ptr() == buf.data_ptr() and len(tr._graphs) == 1
    ce_graph = float(tr.train_step_graphed(*batch)["sem"][0])
    m.store.flat.copy_(snap)                                 # the same parameters, eager, under each setting
    m.mark_weights_dirty()
    ce_new = float(tr.forward_backward(*batch)["sem"][0])
    tr.set_border(10.0, 5.0)
    m.mark_weights_dirty()
    ce_old = float(tr.forward_backward(*batch)["sem"][0])
    torch.cuda.synchronize()
    assert abs(ce_graph - ce_new) <= 1e-5 * abs(ce_new), (ce_graph, ce_new)
    assert abs(ce_graph - ce_old) > 100 * abs(ce_graph - ce_new) + 1e-4, (ce_graph, ce_old)


class _Launches:
    """Stands in for Engine.lib and logs the name of every entry point the step calls, in order."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def test_weight_zero_is_the_step_as_it_was_and_the_term_is_part_of_the_key():
    R, ReSeg, Trainer, class_onehot = _need_model()
    m, batch = _models(R, ReSeg, class_onehot, "instance", seed=6)
    order = [[0, 1], [1, 0]]
    real_lib = m.engine.lib

    def step(tr):
        log = []
        m.engine.lib = _Launches(real_lib, log)
        try:
            tr.forward_backward(*batch, selected_idx=order)
        finally:
            m.engine.lib = real_lib
        torch.cuda.synchronize()
        arena = m.engine.arena
        return log, [(tuple(t.shape), t.dtype) for t in arena.slots[:arena.cursor]] + [arena.stats_cursor]

    def graph_key(tr):
        tr.train_step_graphed(*batch, selected_idx=order)    # first sight: runs eagerly and records the configuration
        torch.cuda.synchronize()
        (key,) = tr._graphs
        return key

    plain = Trainer(m)
    step(plain)                                              # first sight: one-time set-up calls
    log_p, alloc_p = step(plain)
    key_p = graph_key(plain)
    off = Trainer(m, border_weight=0.0, border_sigma=3.0)
    assert m.net.crit.legacy and not m.net.crit.border_on
    log_0, alloc_0 = step(off)
    assert log_0 == log_p and alloc_0 == alloc_p and len(log_p) > 100            # not one launch or allocation more
    assert graph_key(off) == key_p
    assert not any(name in ("isa_edt2_u8", "isa_border_weights", "isa_fill_labels", "isa_labels_from_planes") or
                   name.endswith("_pw") for name in log_0)
    on = Trainer(m, border_weight=10.0)
    log_w, _ = step(on)
    assert graph_key(on) != key_p
    # the shipped combination leaves its 2-class criterion for the K-class one: isa_mask_loss_sums, isa_sem_loss and
    # isa_mask_loss_grad (three calls; the head goes on using the first and the last) make way for the label maps, the
    # transform, the weight map and the three K-class entries (seven calls)
    gone = sorted(set(log_p) - set(log_w))
    new = sorted(set(log_w) - set(log_p))
    assert gone == ["isa_sem_loss"], gone
    assert new == ["isa_border_weights", "isa_edt2_u8", "isa_labels_from_onehot", "isa_labels_from_planes",
                   "isa_sem_loss_k_assemble", "isa_sem_loss_k_grad_pw", "isa_sem_loss_k_sums_pw"], new
    assert len(log_w) == len(log_p) + 4


def test_a_step_without_instance_planes_raises_while_the_term_is_on():
    R, ReSeg, Trainer, class_onehot = _need_model()
    m, (x, sem, ins, n) = _models(R, ReSeg, class_onehot, "semantic3", seed=7)
    tr = Trainer(m, criterion="CE", border_weight=10.0)
    with pytest.raises(ValueError):
        tr.forward_backward(x, sem, ins[:, :0], n)
    with pytest.raises(ValueError):
        Trainer(m, criterion="Lovasz", border_weight=10.0)
    Trainer(m, criterion="CE").forward_backward(x, sem, ins[:, :0], n)            # off: the planes are not looked at
    torch.cuda.synchronize()


def test_validation_costs_take_the_planes_and_use_the_same_map():
    R, ReSeg, Trainer, class_onehot = _need_model()
    m, (x, sem, ins, n) = _models(R, ReSeg, class_onehot, "semantic3", seed=8)
    Trainer(m, criterion="CE", border_weight=10.0, border_sigma=5.0)
    m.eval()
    with torch.no_grad():
        m(False, x)
        costs = m.sem_costs(sem, ins).double().cpu().numpy()            # before the next forward
        logits = m.net.to_nchw(m._last_sem).double().cpu().numpy()
        with pytest.raises(ValueError):
            m.sem_costs(sem)
    lab = _label_map(ins)
    d1, d2, _ = dn.edt2(lab)
    ce = _ce_restatement(logits, sem.argmax(1).numpy(), dn.border_weights(lab, d1, d2, 10.0, 5.0))
    assert abs(costs[0] - ce) <= 1e-4 and costs[1] == 0.0, (costs, ce)
