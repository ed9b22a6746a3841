#!/usr/bin/env python3
"""Time of the discriminative embedding loss, forward + gradient, against the same formulas in torch ops on the device.

Inputs already on the device: an embedding NHWC [B,H,W,C = 24] (bf16, then fp32), a uint8 label map [B,H,W] of 8 instances
an image and the object counts; the 'full' form (var + dist + 0.001 reg on plain means), L2 norm.
  (a) kernels : LabelOps.disc_loss - sums, means, hinge, assemble - and isa_disc_grad; d emb in the embedding's dtype;
  (b) torch   : one-hot matmul for the means, gathered means for the pull hinge, pairwise distances for the push hinge,
                autograd for d emb (fp32 from the stored embedding).  (The reference's own formulation expands
                [B, L, 32, C]: 3 GB at this size.)
The two are called alternately, --calls times each after --warmup, every call timed with events of its own; the median is
reported.  Then a whole training step (B, size, bf16, instance head on) with and without the loss, both as hipGraph replays,
same protocol.  No threshold: the script reports.  Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import isa_amd  # noqa: F401,E402
from isa_amd.engine import Act, Arena  # noqa: E402
from isa_amd.labelmaps import DiscCriterion, LabelOps  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402
from isa_amd.trainer import Trainer  # noqa: E402

K_OBJ, DELTA_V, DELTA_D = 8, 2.9, 3.0


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


def torch_disc(emb, labels, C):
    """The 'full' form on every instance 1..K_OBJ (all present), fp32 autograd."""
    B = emb.shape[0]
    x = emb[..., :C].float().reshape(B, -1, C).requires_grad_(True)
    lab = labels.reshape(B, -1).long()
    onehot = torch.nn.functional.one_hot(lab, K_OBJ + 1)[..., 1:].float()             # [B, L, K]
    cnt = onehot.sum(1)                                                                # [B, K]
    mu = torch.bmm(onehot.transpose(1, 2), x) / cnt[..., None]                         # [B, K, C]
    fg = lab > 0
    own = torch.gather(mu, 1, (lab - 1).clamp_min(0)[..., None].expand(-1, -1, C))
    h = ((x - own).norm(dim=2) - DELTA_V).clamp_min(0) * fg
    var = ((h * h).sum(1) / fg.sum(1)).mean()
    d = (mu[:, :, None] - mu[:, None]).norm(dim=3)
    t = (2 * DELTA_D - d).clamp_min(0) * (1 - torch.eye(K_OBJ, device=x.device))
    dist = ((t * t).sum((1, 2)) / (K_OBJ * (K_OBJ - 1))).mean()
    reg = mu.norm(dim=2).mean(1).mean()
    loss = var + dist + 0.001 * reg
    loss.backward()
    return loss.detach(), x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disc.py needs the GPU"
    B, S, C = opt.batch, opt.size, opt.channels
    lines = ["disc bench: %s, B=%d, %d x %d, C=%d, %d instances an image, form 'full', L2; median of %d alternating calls after "
             "%d warm-up, one event pair per call" % (torch.cuda.get_device_name(0), B, S, S, C, K_OBJ, opt.calls, opt.warmup)]
    arena = Arena(torch.device("cuda", torch.cuda.current_device()))     # as in a training step: the scratch is reused
    ops = LabelOps(alloc=arena.alloc)
    crit = DiscCriterion("cuda")
    crit.set(1.0, DELTA_V, DELTA_D, 2, "full")
    g = torch.Generator(device="cuda").manual_seed(5)
    labels = torch.randint(0, K_OBJ + 1, (B, S // 8, S // 8), generator=g, device="cuda", dtype=torch.int32)
    labels = labels.repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.uint8).contiguous()      # 8 x 8 blocks
    n_obj = torch.full((B,), K_OBJ, dtype=torch.int32, device="cuda")
    centres = torch.randn((K_OBJ + 1, C), generator=g, device="cuda") * 0.3
    base = torch.randn((B, S, S, C), generator=g, device="cuda") * 0.6 + centres[labels.long()]
    for dtype in (torch.bfloat16, torch.float32):
        emb = base.to(dtype).contiguous()
        a, da = Act(emb, 0, C), Act(torch.empty_like(emb), 0, C)
        res = {}

        def kernels():
            arena.reset()
            res["scal"], _, grad = ops.disc_loss(a, labels.view(B, -1), 32, n_obj, crit.cfg, crit.norm)
            grad(da, 0)

        def baseline():
            res["ref"], res["ref_grad"] = torch_disc(emb, labels, C)

        t_k, t_t = alternate([kernels, baseline], opt.calls, opt.warmup)
        got, ref = float(res["scal"][0]), float(res["ref"])
        gerr = float((da.buf.float().reshape(B, -1, C) - res["ref_grad"]).norm() / res["ref_grad"].norm())
        passes = B * S * S * C * emb.element_size()
        lines.append("%-8s (a) kernels %8.3f ms   (b) torch one-hot matmul + autograd %8.3f ms   (b) / (a) %6.2f   loss %.6f vs "
                     "%.6f, d emb rel L2 %.1e; one pass over the embedding = %.1f MB"
                     % (str(dtype)[6:], t_k, t_t, t_t / t_k, got, ref, gerr, passes / 1e6))
    del ops, arena
    torch.cuda.empty_cache()
    if not opt.no_step:
        from isa_amd.data import synth_batch
        x, sem_t, ins, n = synth_batch(B, S, S, seed=100)
        x, sem_t, ins = x.cuda(), sem_t.cuda(), ins.cuda()
        sel = [list(range(int(k))) for k in n.view(-1)]
        steps = []
        for w in (0.0, 1.0):
            m = ReSeg(2, True, dtype=torch.bfloat16)
            m.reset_parameters(seed=23)
            m.train()
            tr = Trainer(m, disc_weight=w)
            steps.append(lambda tr=tr: tr.train_step_graphed(x, sem_t, ins, n, selected_idx=sel))
        t_0, t_1 = alternate(steps, opt.calls, opt.warmup)
        lines.append("train step (bf16, instance head on, hipGraph replay): without the loss %8.3f ms   with it %8.3f ms   "
                     "difference %+.3f ms" % (t_0, t_1, t_1 - t_0))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
