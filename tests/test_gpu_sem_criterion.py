"""GPU: the K-class semantic criterion (isa_sem_loss_k_*, isa_labels_from_onehot, isa_collate_targets_k) and the
trainer wired to it (Trainer(criterion, class_weights, optimize_bg), ReSeg(n_classes=K)).

The yardstick is the float64 restatement of tests/test_sem_criterion_ref.py, itself pinned to the reference's dice_loss
and CrossEntropyLoss(weight).  Bounds: fp32 logits - loss <= 1e-5 relative, gradient <= 1e-5 relative L2; bf16 logits -
the restatement on the same bf16-rounded logits, loss <= 1e-5 relative, gradient (stored in bf16) <= 8e-3 relative L2."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from test_sem_criterion_ref import criterion, criterion_grad  # noqa: E402

CRITERIA = ("CE", "Dice", "Multi")


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L


def _rup8(k):
    return (k + 7) // 8 * 8


def _desc(L, buf, n, h, w, c, dtype):
    return L.IsaTensor(buf.data_ptr(), n, h, w, c, buf.shape[-1], L.dtype_code(dtype), 1)


def _cfg(crit, weights, bg, K):
    w = [1.0] * K if weights is None else list(weights)
    return torch.tensor([float(crit in ("CE", "Multi")), float(crit in ("Dice", "Multi")), float(bg), 0.0] + w,
                        dtype=torch.float32, device="cuda")


def _inputs(B, K, H, W, dtype, seed):
    """NHWC logits with NaN in the ld padding (must never be read as a class), labels uint8, the float64 logits the
    kernels actually see (NCHW) and the labels as int64 numpy."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, H, W, K, generator=g, dtype=torch.float64) * 2.5
    lg[..., 0] += 0.5
    buf = torch.full((B, H, W, _rup8(K)), float("nan"), dtype=dtype)
    buf[..., :K] = lg.to(dtype)
    seen = buf[..., :K].double().permute(0, 3, 1, 2).contiguous().numpy()
    lab = torch.randint(0, K, (B, H, W), generator=g, dtype=torch.int64)
    return buf.cuda(), lab.to(torch.uint8).cuda(), seen, lab.numpy()


def _run(L, buf, lab, cfg, B, K, H, W, dtype, dx=None, acc=0):
    lib = L.lib()
    x = _desc(L, buf, B, H, W, K, dtype)
    sums = torch.zeros(3 * B * K + 2, device="cuda")
    coef = torch.full((3 * B * K + 1,), float("nan"), device="cuda")
    scal = torch.full((2,), float("nan"), device="cuda")
    if dx is None:
        dx = torch.full_like(buf, float("nan"))
    d = _desc(L, dx, B, H, W, K, dtype)
    s = L.stream_ptr()
    L.check(lib.isa_sem_loss_k_sums(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(sums), s), "sums")
    L.check(lib.isa_sem_loss_k_assemble(L.ptr(sums), L.ptr(cfg), B, K, L.ptr(coef), L.ptr(scal), s), "assemble")
    L.check(lib.isa_sem_loss_k_grad(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(coef), C.byref(d), acc, s), "grad")
    torch.cuda.synchronize()
    return scal.cpu().double().numpy(), dx


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [2, 3, 8, 12, 21, 32])       # every class width of the kernels: 8, 16, 24, 32
def test_loss_kernels_match_the_restatement(K, dtype):
    L = _lib()
    gbound = 1e-5 if dtype == torch.float32 else 8e-3
    worst = 0.0
    for B, H, W in ((3, 20, 27), (16, 17, 33)):          # H*W = 540, 561: never a multiple of the 256-pixel tile
        buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=K * 100 + B)
        rs = np.random.RandomState(K + B)
        for crit in CRITERIA:
            for weights in (None, list(rs.uniform(0.2, 2.0, K))):
                for bg in (False, True):
                    cfg = _cfg(crit, weights, bg, K)
                    scal, dx = _run(L, buf, lab, cfg, B, K, H, W, dtype)
                    ce, dice = criterion(seen, lab_np, crit, weights, bg)
                    tag = (K, B, crit, weights is not None, bg)
                    for got, ref in ((scal[0], ce), (scal[1], dice)):
                        if ref is None:
                            assert got == 0.0, tag
                        else:
                            assert abs(got - ref) <= 1e-5 * max(abs(ref), 1e-3), (tag, got, ref)
                    ref_g = criterion_grad(seen, lab_np, crit, weights, bg)
                    got_g = dx[..., :K].double().permute(0, 3, 1, 2).cpu().numpy()
                    e = _rel_l2(got_g, ref_g)
                    worst = max(worst, e)
                    assert e <= gbound, (tag, e)
                    assert torch.isnan(dx[..., K:]).all(), "the ld padding of d logits must stay untouched"
    print("K=%d %s: worst gradient rel-L2 %.2e" % (K, dtype, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_grad_accumulates(dtype):
    L = _lib()
    B, K, H, W = 2, 5, 9, 31
    buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=7)
    cfg = _cfg("Multi", [1.0, 2.0, 0.5, 1.0, 3.0], True, K)
    old = torch.randn(B, H, W, _rup8(K), generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    _, fresh = _run(L, buf, lab, cfg, B, K, H, W, dtype)
    _, acc = _run(L, buf, lab, cfg, B, K, H, W, dtype, dx=old.clone(), acc=1)
    want = old[..., :K].float() + fresh[..., :K].float()
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert float((acc[..., :K].float() - want).abs().max()) <= tol
    assert torch.equal(acc[..., K:], old[..., K:])


def test_kernels_refuse_bad_arguments():
    L = _lib()
    lib = L.lib()
    B, K, H, W = 2, 3, 8, 8
    buf, lab, _, _ = _inputs(B, K, H, W, torch.float32, seed=1)
    cfg, sums = _cfg("Multi", None, False, K), torch.zeros(3 * B * K + 2, device="cuda")
    s = L.stream_ptr()
    bad_k = _desc(L, torch.zeros(B, H, W, 40, device="cuda"), B, H, W, 33, torch.float32)   # K > 32
    assert lib.isa_sem_loss_k_sums(C.byref(bad_k), L.ptr(lab), L.ptr(cfg), L.ptr(sums), s) == -1
    x = _desc(L, buf, B, H, W, K, torch.float32)
    assert lib.isa_sem_loss_k_sums(C.byref(x), None, L.ptr(cfg), L.ptr(sums), s) == -1
    assert lib.isa_sem_loss_k_assemble(L.ptr(sums), L.ptr(cfg), B, 1, L.ptr(sums), L.ptr(sums), s) == -1
    other = _desc(L, torch.zeros(B, H, W, 8, dtype=torch.bfloat16, device="cuda"), B, H, W, K, torch.bfloat16)
    assert lib.isa_sem_loss_k_grad(C.byref(x), L.ptr(lab), L.ptr(cfg), L.ptr(sums), C.byref(other), 0, s) == -1
    assert lib.isa_labels_from_onehot(None, B, K, H * W, L.ptr(lab), None, s) == -1
    assert lib.isa_collate_targets_k(None, L.ptr(lab), B, H, W, 4, K, None, None, None, s) == -1
    assert float(sums.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------- (b)
def test_two_class_multi_ties_to_the_shipped_kernels():
    L = _lib()
    lib = L.lib()
    B, K, H, W = 4, 2, 37, 41
    buf, lab, seen, lab_np = _inputs(B, K, H, W, torch.float32, seed=11)
    scal, dx = _run(L, buf, lab, _cfg("Multi", None, False, K), B, K, H, W, torch.float32)
    onehot = torch.from_numpy(np.eye(2, dtype=np.int64)[lab_np]).permute(0, 3, 1, 2).contiguous().cuda()
    x = _desc(L, buf, B, H, W, K, torch.float32)
    sums, coef, s2 = torch.zeros(8 * B, device="cuda"), torch.zeros(4 * B, device="cuda"), torch.zeros(2, device="cuda")
    dref = torch.full_like(buf, float("nan"))
    d = _desc(L, dref, B, H, W, K, torch.float32)
    s = L.stream_ptr()
    L.check(lib.isa_mask_loss_sums(C.byref(x), None, L.ptr(onehot), L.ptr(sums), s), "isa_mask_loss_sums")
    L.check(lib.isa_sem_loss(L.ptr(sums), B, L.ptr(coef), L.ptr(s2), s), "isa_sem_loss")
    L.check(lib.isa_mask_loss_grad(C.byref(x), None, L.ptr(onehot), L.ptr(coef), C.byref(d), 0, s), "isa_mask_loss_grad")
    torch.cuda.synchronize()
    ref = s2.cpu().double().numpy()
    assert np.all(np.abs(scal - ref) <= 1e-6 * np.abs(ref)), (scal, ref)
    assert _rel_l2(dx[..., :2].double().cpu().numpy(), dref[..., :2].double().cpu().numpy()) <= 1e-6


# ---------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("K,n_ins", [(2, 32), (3, 32), (21, 5), (32, 16)])
def test_collate_and_labels_are_bit_exact(K, n_ins):
    L = _lib()
    lib = L.lib()
    n, h, w = 3, 19, 23
    rs = np.random.RandomState(K)
    sem = rs.randint(0, K, (n, h, w)).astype(np.uint8)
    ins = rs.randint(0, 2, (n, h, w, n_ins)).astype(np.uint8)
    sem_d, ins_d = torch.from_numpy(sem).cuda(), torch.from_numpy(ins).cuda()
    ins_out = torch.full((n, n_ins, h, w), -7, dtype=torch.int64, device="cuda")
    sem_out = torch.full((n, K, h, w), -7, dtype=torch.int64, device="cuda")
    lab_out = torch.full((n, h, w), 255, dtype=torch.uint8, device="cuda")
    s = L.stream_ptr()
    L.check(lib.isa_collate_targets_k(L.ptr(ins_d), L.ptr(sem_d), n, h, w, n_ins, K, L.ptr(ins_out), L.ptr(sem_out),
                                      L.ptr(lab_out), s), "isa_collate_targets_k")
    onehot_np = np.eye(K, dtype=np.int64)[sem].transpose(0, 3, 1, 2)
    torch.cuda.synchronize()
    assert np.array_equal(sem_out.cpu().numpy(), onehot_np)
    assert np.array_equal(ins_out.cpu().numpy(), ins.astype(np.int64).transpose(0, 3, 1, 2))
    assert np.array_equal(lab_out.cpu().numpy(), sem)
    # one-hot -> labels / argmax map; a target with ties and all-zero rows takes the first maximum, like torch.argmax
    oh = rs.randint(0, 2, (n, K, h, w)).astype(np.int64)
    for src in (onehot_np, oh):
        src_d = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        lab = torch.full((n, h, w), 255, dtype=torch.uint8, device="cuda")
        amap = torch.full((n, h * w), float("nan"), device="cuda")
        L.check(lib.isa_labels_from_onehot(L.ptr(src_d), n, K, h * w, L.ptr(lab), L.ptr(amap), s), "labels")
        torch.cuda.synchronize()
        want = src.argmax(1)
        assert np.array_equal(lab.cpu().numpy(), want.astype(np.uint8))
        assert np.array_equal(amap.cpu().numpy(), want.reshape(n, -1).astype(np.float32))
        assert np.array_equal(want, torch.from_numpy(np.ascontiguousarray(src)).argmax(1).numpy())


# ---------------------------------------------------------------------------------------------------------- (d), (e)
def _need_model():
    _lib()
    import reseg_ref as R
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    from isa_amd.data import class_onehot
    return R, ReSeg, Trainer, class_onehot


def _three_class_sd(R):
    sd = R.synth_state_dict(23, use_instance_seg=False)
    rs = np.random.RandomState(77)
    sd["sem_seg_output.weight"] = torch.from_numpy((rs.standard_normal((3, 32, 1, 1)) * 0.25).astype(np.float32))
    sd["sem_seg_output.bias"] = torch.from_numpy(rs.uniform(-0.1, 0.1, 3).astype(np.float32))
    return sd


def _torch_criterion(logits, onehot, crit, weights, bg):
    """The restatement in torch float64 (autograd carries it back through the oracle network)."""
    K = logits.shape[1]
    w = torch.ones(K, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    cost = 0
    if crit in ("CE", "Multi"):
        cost = cost + torch.nn.functional.cross_entropy(logits.permute(0, 2, 3, 1).reshape(-1, K),
                                                        onehot.argmax(1).reshape(-1), weight=w)
    if crit in ("Dice", "Multi"):
        p, g = torch.softmax(logits, 1), onehot.double()
        D = (2 * (p * g).sum((2, 3)) + 1) / (p.sum((2, 3)) + g.sum((2, 3)) + 1)
        Cs = list(range(0 if bg else 1, K))
        wn = len(Cs) * w[Cs] / w[Cs].sum()
        cost = cost + (1 - (wn[None] * D[:, Cs]).mean(1)).mean()
    return cost


@pytest.mark.parametrize("crit,weights,bg", [("CE", [0.4, 1.3, 2.2], False), ("Dice", None, True)])
def test_three_class_step_matches_float64_autograd(crit, weights, bg):
    R, ReSeg, Trainer, class_onehot = _need_model()
    x, _, ins, n = R.synth_batch(2, 64, 64, seed=1)
    sem = class_onehot(ins, 3)
    sd = _three_class_sd(R)
    m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(sd)
    m.train()
    tr = Trainer(m, criterion=crit, class_weights=weights, optimize_bg=bg)
    out = tr.forward_backward(x, sem, ins, n)
    logits = m.net.to_nchw(m._last_sem).double().cpu()
    scal = out["sem"].double().cpu()
    torch.cuda.synchronize()
    P = {k: (v.double().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v)
         for k, v in sd.items()}
    ref = R.reseg_forward(P, x.double(), sem, use_instance_seg=False, ctx=R.Ctx(bn_train=True, training=True))
    lref = ref["sem_out"]
    assert float((logits - lref.detach()).abs().max()) <= 1e-4 * float(lref.detach().abs().max())
    ce, dice = criterion(lref.detach().numpy(), sem.argmax(1).numpy(), crit, weights, bg)
    if ce is not None:
        assert abs(float(scal[0]) - ce) < 1e-4 and float(scal[1]) == 0.0
    if dice is not None:
        assert abs(float(scal[1]) - dice) < 1e-4 and float(scal[0]) == 0.0
    _torch_criterion(lref, sem, crit, weights, bg).backward()
    errs = {}
    gmax = max(float(v.grad.norm()) for v in P.values() if getattr(v, "grad", None) is not None)
    for k, v in P.items():
        if getattr(v, "grad", None) is None or float(v.grad.norm()) <= 1e-6 * gmax:
            continue
        errs[k] = float((m.store.gview(k).double().cpu() - v.grad).norm() / v.grad.norm())
    assert len(errs) > 100 and "sem_seg_output.weight" in errs
    worst = max(errs, key=errs.get)
    med = float(np.median(list(errs.values())))
    print("3-class %s step vs float64: %d tensors, worst rel-L2 %.2e (%s), median %.2e"
          % (crit, len(errs), errs[worst], worst, med))
    # the bounds of test_gpu_train.test_backbone_gradients_tight_vs_oracle_f64
    assert errs[worst] <= 1e-4 and med <= 1e-5, (worst, errs[worst], med)


def test_graph_replay_follows_in_place_class_weights():
    R, ReSeg, Trainer, class_onehot = _need_model()
    x, _, ins, n = R.synth_batch(2, 64, 64, seed=2)
    sem = class_onehot(ins, 3)
    m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(_three_class_sd(R))
    m.train()
    w0, w1 = [0.4, 1.3, 2.2], [3.0, 0.2, 0.7]
    tr = Trainer(m, criterion="CE", class_weights=w0)
    buf = tr.class_weights
    tr.train_step_graphed(x, sem, ins, n)                    # eager (configuration recorded)
    tr.train_step_graphed(x, sem, ins, n)                    # captured, replayed
    assert tr._graphs and list(tr._graphs.values())[0]["state"] == "ready"
    snap = m.store.flat.clone()
    tr.class_weights.copy_(torch.tensor(w1))                 # in place: the graph reads this buffer
    assert tr.class_weights.data_ptr() == buf.data_ptr()
    ce_graph = float(tr.train_step_graphed(x, sem, ins, n)["sem"][0])
    grad_graph = m.store.grad[:m.store.n_train].clone()
    m.store.flat.copy_(snap)                                 # the same parameters, eager, under each weight set
    m.mark_weights_dirty()
    ce_new = float(tr.forward_backward(x, sem, ins, n)["sem"][0])
    grad_new = m.store.grad[:m.store.n_train].clone()
    tr.class_weights.copy_(torch.tensor(w0))
    m.mark_weights_dirty()
    ce_old = float(tr.forward_backward(x, sem, ins, n)["sem"][0])
    grad_old = m.store.grad[:m.store.n_train].clone()
    torch.cuda.synchronize()
    assert abs(ce_graph - ce_new) <= 1e-5 * abs(ce_new), (ce_graph, ce_new)
    assert abs(ce_graph - ce_old) > 100 * abs(ce_graph - ce_new) + 1e-4, (ce_graph, ce_old)
    # two runs of one step differ by the float-atomic summation order, which can flip a ReLU6 threshold upstream:
    # test_gpu_train.test_graph_replayed_step_matches_eager_step allows 2e-2 for that; the weight change moves the
    # gradient by far more
    d_new = float((grad_graph - grad_new).norm() / grad_new.norm())
    d_old = float((grad_graph - grad_old).norm() / grad_old.norm())
    assert d_new <= 2e-2 and d_old > 10 * d_new, (d_new, d_old)


def test_instance_head_with_class_weights():
    R, ReSeg, Trainer, _ = _need_model()
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=3)
    m = ReSeg(2, True, dtype=torch.float32)
    m.load_state_dict(R.synth_state_dict(23, True))
    m.train()
    m.head.drop_rate = 0.0
    weights = [0.3, 1.7]
    tr = Trainer(m, criterion="Multi", class_weights=weights)
    assert tr.class_weights is not None
    out = tr.forward_backward(x, sem, ins, n)
    logits = m.net.to_nchw(m._last_sem).double().cpu().numpy()
    scal = out["sem"].double().cpu().numpy()
    head = out["head"].cpu()
    torch.cuda.synchronize()
    ce, dice = criterion(logits, sem.argmax(1).numpy(), "Multi", weights, False)
    unweighted, _ = criterion(logits, sem.argmax(1).numpy(), "Multi", None, False)
    assert abs(scal[0] - ce) <= 1e-5 * ce and abs(scal[1] - dice) <= 1e-5 * dice
    assert abs(ce - unweighted) > 1e-3                     # the weights matter
    assert torch.isfinite(head[1:]).all() and torch.isfinite(m.store.grad[:m.store.n_train]).all()


def test_n_classes_guards():
    R, ReSeg, Trainer, _ = _need_model()
    shipped = Trainer(ReSeg(2, use_instance_seg=False))   # the shipped criterion keeps its 2-class kernels
    assert shipped.model.net.crit.legacy and shipped.class_weights is None
    with pytest.raises(ValueError):
        ReSeg(3, use_instance_seg=True)
    with pytest.raises(ValueError):
        ReSeg(33, use_instance_seg=False)
    m = ReSeg(3, use_instance_seg=False)
    with pytest.raises(ValueError):
        Trainer(m, criterion="CE", class_weights=[1.0, 2.0])
