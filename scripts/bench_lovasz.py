#!/usr/bin/env python3
"""Time of the Lovasz-Softmax criterion, forward + backward, against the same loss written with torch ops on the device.

Inputs already on the device: logits NHWC [B,H,W,ld = rup(K, 8)] bf16 and a uint8 label map [B,H,W]; batch-wide segments,
every class counted (lovasz_softmax's defaults).
  (a) kernels : Network.sem_loss with the "Lovasz" criterion and its backward closure - keys, segmented sort, coefficients
                (per class group), assemble, gradient; d logits in bf16;
  (b) torch   : softmax, then per class torch.sort(descending) of the errors, cumsum, the Jaccard differences of
                lovasz_grad, a dot product; autograd for d logits (fp32 from the bf16 logits).
The two are called alternately, --calls times each after --warmup, every call timed with events of its own; the median is
reported.  Then a whole training step (B, size, bf16, instance head on) with --criterion CELovasz next to the shipped Multi
step, both as hipGraph replays, same protocol.  Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import isa_amd  # noqa: F401,E402
from isa_amd.engine import Act  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402
from isa_amd.trainer import Trainer  # noqa: E402


def timed_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(fns, calls, warmup):
    """Median ms of each function, called in turn."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for i, f in enumerate(fns):
            ts[i].append(timed_ms(f))
    return [statistics.median(t) for t in ts]


def torch_lovasz(logits, labels, K):
    x = logits[..., :K].float().requires_grad_(True)
    p = torch.softmax(x, -1).reshape(-1, K)
    lab = labels.reshape(-1)
    loss = 0
    for c in range(K):
        fg = (lab == c).float()
        err = (fg - p[:, c]).abs()
        es, perm = torch.sort(err, 0, descending=True)
        fgs = fg[perm]
        gts = fgs.sum()
        jac = 1.0 - (gts - fgs.cumsum(0)) / (gts + (1 - fgs).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        loss = loss + torch.dot(es, jac)
    loss = loss / K
    loss.backward()
    return loss.detach(), x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--classes", default="2,8,32")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lovasz.py needs the GPU"
    B, S = opt.batch, opt.size
    lines = ["lovasz bench: %s, B=%d, %d x %d, bf16 logits; median of %d alternating calls after %d warm-up, one event pair "
             "per call" % (torch.cuda.get_device_name(0), B, S, S, opt.calls, opt.warmup)]
    for K in [int(v) for v in opt.classes.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(K)
        ld = (K + 7) // 8 * 8
        logits = (torch.randn((B, S, S, ld), generator=g, device="cuda") * 2.5).to(torch.bfloat16).contiguous()
        labels = torch.randint(0, K, (B, S, S), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8).contiguous()
        m = ReSeg(K, use_instance_seg=False, dtype=torch.bfloat16)
        m.set_criterion("Lovasz", None, True)
        E, sem = m.engine, Act(logits, 0, K)
        res = {}

        def kernels():
            E.begin(bn_train=True, record=True, key=("bench-lovasz", K))
            res["loss"] = m.net.sem_loss(sem, None, labels)
            bwd, _ = E.tape[-1]
            bwd()

        def baseline():
            res["ref"], res["ref_grad"] = torch_lovasz(logits, labels, K)

        t_k, t_t = alternate([kernels, baseline], opt.calls, opt.warmup)
        got, ref = float(res["loss"][2]), float(res["ref"])
        dg = E.grads.grad_of(sem).buf[..., :K].float()
        gerr = float((dg - res["ref_grad"]).norm() / res["ref_grad"].norm())
        from isa_amd.network import lovasz_class_group
        lines.append("K=%-2d (a) kernels %8.3f ms   (b) torch sort + cumsum + autograd %8.3f ms   (b) / (a) %5.2f   loss %.6f vs "
                     "%.6f, d logits (bf16 vs torch fp32) rel L2 %.1e, classes per sort group %d"
                     % (K, t_k, t_t, t_t / t_k, got, ref, gerr, lovasz_class_group(K, B * S * S, True)))
        del m, logits, labels
        torch.cuda.empty_cache()
    if not opt.no_step:
        from isa_amd.data import synth_batch
        x, sem_t, ins, n = synth_batch(B, S, S, seed=100)
        x, sem_t, ins = x.cuda(), sem_t.cuda(), ins.cuda()
        sel = [list(range(int(k))) for k in n.view(-1)]
        steps = []
        for crit in ("Multi", "CELovasz"):
            m = ReSeg(2, True, dtype=torch.bfloat16)
            m.reset_parameters(seed=23)
            m.train()
            tr = Trainer(m, criterion=crit)
            steps.append(lambda tr=tr: tr.train_step_graphed(x, sem_t, ins, n, selected_idx=sel))
        t_m, t_l = alternate(steps, opt.calls, opt.warmup)
        lines.append("train step (instance head on, hipGraph replay): Multi %8.3f ms   CELovasz %8.3f ms   difference %+.3f ms"
                     % (t_m, t_l, t_l - t_m))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
