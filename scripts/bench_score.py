#!/usr/bin/env python3
"""Time of scoring a batch of instance predictions: the host path against ReSeg.score_instances.

Inputs, the same for both sides and already on the device (where ReSeg.segment leaves them): predicted labels uint8
[B,H,W] and counts, the compact ground truth (instance planes uint8 [B,H,W,32], semantic map uint8 [B,H,W]) and the
predicted foreground map fp32 [B,1,H,W].  Two label distributions: "background" (about 95 % of the pixels are
background in both maps, the rest spread over 32 objects: what leaf images look like) and "uniform" (every pixel drawn
uniformly from 0..32 in both maps).
  (a) host  : .cpu() of labels and targets, planes -> label map with numpy, evaluate.calc_sbd and calc_dice per image
              (what scoring a batch cost before the kernels existed); host clock, median of --host-calls calls;
  (b) device: score_instances(check=False) to the finished [B,8] tensor - isa_labels_from_planes x2,
              isa_label_pair_hist x2, isa_instance_scores x2, isa_labels_from_onehot none (compact targets) - timed with
              events over --calls calls after --warmup.
Then isa_label_pair_hist alone (33 x 33 counters, events over --calls calls) in its two modes: ISA_HIST_AGGREGATE (the
dominant pair of a wave counted with ballot + popcount, equal consecutive pairs of a lane merged) and ISA_HIST_NAIVE
(one LDS atomic per pixel).  Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import isa_amd  # noqa: F401,E402
from evaluate import calc_dice, calc_sbd  # noqa: E402
from isa_amd import lib as L  # noqa: E402
from isa_amd.labelmaps import LabelOps  # noqa: E402

K = 32


def make_inputs(B, size, dist, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (B, size, size)
    draw = lambda: torch.randint(0, K + 1, shape, generator=g, device="cuda", dtype=torch.int32)
    gt, pred = draw(), draw()
    if dist == "background":
        keep = torch.rand(shape, generator=g, device="cuda") < 0.05
        gt, pred = gt * keep, pred * keep
    gt, pred = gt.to(torch.uint8), pred.to(torch.uint8)
    planes = (gt.unsqueeze(-1) == torch.arange(1, K + 1, device="cuda", dtype=torch.uint8)).to(torch.uint8).contiguous()
    sem_t = (gt != 0).to(torch.uint8)
    sem_arg = (pred != 0).float().unsqueeze(1).contiguous()
    n_gt = torch.full((B,), K, dtype=torch.int64, device="cuda")
    n_pred = torch.full((B,), K, dtype=torch.int32, device="cuda")
    return pred.contiguous(), n_pred, planes, n_gt, sem_arg, sem_t


def host_path(pred, n_pred, planes, n_gt, sem_arg, sem_t):
    lab, pl, fg_p, fg_t = pred.cpu().numpy(), planes.cpu().numpy(), sem_arg.cpu().numpy()[:, 0] > 0.5, sem_t.cpu().numpy() == 1
    n_p, n_g = n_pred.cpu().numpy(), n_gt.cpu().numpy()
    out = []
    for i in range(lab.shape[0]):
        nz = pl[i] != 0
        gt = np.where(nz.any(-1), nz.argmax(-1) + 1, 0)
        out.append((calc_sbd(gt, lab[i]), abs(int(n_g[i]) - int(n_p[i])), calc_dice(fg_t[i], fg_p[i])))
    return out


def event_us(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls * 1e3


def hist_alone(a, b, na, nb, mode, calls, warmup):
    lib = L.lib()
    n, Lp = a.shape[0], a[0].numel()
    hist = torch.empty(n * na * nb, dtype=torch.int32, device="cuda")
    oob = torch.empty(n, dtype=torch.int32, device="cuda")
    st = L.stream_ptr()
    call = lambda: L.check(lib.isa_label_pair_hist(L.ptr(a), L.ptr(b), n, Lp, na, nb, L.ptr(hist), L.ptr(oob), mode, st),
                           "isa_label_pair_hist")
    us = event_us(call, calls, warmup)
    return us, hist.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_score.py needs the GPU"
    B = opt.batch
    lines = ["score bench: %s, B=%d, %d objects; host: median of %d calls (host clock), device: events over %d calls after "
             "%d warm-up" % (torch.cuda.get_device_name(0), B, K, opt.host_calls, opt.calls, opt.warmup)]
    m = LabelOps()
    for size in [int(v) for v in opt.sizes.split(",")]:
        hist_us = {}
        for dist in ("background", "uniform"):
            inp = make_inputs(B, size, dist, seed=size)
            pred, n_pred, planes, n_gt, sem_arg, sem_t = inp
            dev = lambda: m.score_instances(pred, n_pred, planes, n_gt, sem_arg, sem_t, max_objects=K, check=False)
            out = dev().cpu().numpy()
            ts = []
            for _ in range(opt.host_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = host_path(*inp)
                ts.append((time.perf_counter() - t0) * 1e3)
            worst = max(max(abs(out[i, 2] - host[i][0]), abs(out[i, 6] - host[i][2])) for i in range(B))
            assert worst <= 1e-12 and int(m.last_score_oob.sum()) == 0, worst
            t_host = statistics.median(ts)
            t_dev = event_us(dev, opt.calls, opt.warmup) / 1e3
            lines.append("%4d x %-4d %-10s (a) host %9.2f ms   (b) device %7.3f ms   host / device %7.1f   (SBD and FG Dice "
                         "agree to %.1e)" % (size, size, dist, t_host, t_dev, t_host / t_dev, worst))
            gt = torch.empty((B, size * size), dtype=torch.uint8, device="cuda")
            L.check(L.lib().isa_labels_from_planes(L.ptr(planes), L.PLANES_U8_NHWK, B, K, size * size, L.ptr(gt),
                                                   L.stream_ptr()), "isa_labels_from_planes")
            res = {}
            for name, mode in (("aggregate", L.HIST_AGGREGATE), ("naive", L.HIST_NAIVE)):
                us, h = hist_alone(gt, pred.view(B, -1), K + 1, K + 1, mode, opt.calls, opt.warmup)
                res[name] = h
                hist_us[(dist, name)] = us
                lines.append("%4d x %-4d %-10s isa_label_pair_hist alone, %-9s: %8.1f us per call (memset + kernel) = %6.0f GB/s "
                             "of the %d map bytes" % (size, size, dist, name, us, 2 * B * size * size / us / 1e3,
                                                      2 * B * size * size))
            assert torch.equal(res["aggregate"], res["naive"])
        for name in ("aggregate", "naive"):
            lines.append("%4d x %-4d isa_label_pair_hist %-9s: background / uniform = %.2f"
                         % (size, size, name, hist_us[("background", name)] / hist_us[("uniform", name)]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
