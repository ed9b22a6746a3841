#!/usr/bin/env python3
"""Time of the confusion matrix of a batch of K-class semantic predictions, three ways.

Inputs, the same for all and already on the device: logits NHWC [B,H,W,ld = rup(K, 8)] (bf16 or fp32; where the network's
semantic head leaves them) and a uint8 label map [B,H,W].  Two label distributions: "background" (at least 95 % of the
pixels have label 0 AND predict class 0: what semantic maps of small objects look like) and "uniform" (labels and logits
drawn uniformly).
  (a) host    : what scoring cost before the kernels existed - isa_softmax_nchw, the fp32 [B,K,H,W] download of
                Model.predict, np.argmax and np.bincount per image; host clock, --host-calls calls, "background" labels
                only (its cost does not depend on the labels);
  (b) unfused : what the older entry points allow on the device - isa_chan_argmax (a map of the logits' dtype, ld 8),
                a cast to uint8, isa_label_pair_hist (ISA_HIST_AGGREGATE);
  (c) fused   : isa_sem_confusion writing the confusion matrix and the uint8 class map in one pass over the logits.
Then isa_sem_confusion alone, counters only, against the bytes it must read (logits + labels).
(b), (c) and the last are timed with events over --calls calls after --warmup; the three confusion matrices must be equal.
Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import isa_amd  # noqa: F401,E402
from isa_amd import lib as L  # noqa: E402


def make_inputs(B, size, K, dtype, dist, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = (K + 7) // 8 * 8
    logits = torch.randn((B, size, size, ld), generator=g, device="cuda", dtype=torch.float32)
    labels = torch.randint(0, K, (B, size, size), generator=g, device="cuda", dtype=torch.int32)
    if dist == "background":
        bg = torch.rand((B, size, size), generator=g, device="cuda") >= 0.04
        labels = labels * ~bg
        logits[..., 0] += 20.0 * bg                              # class 0 wins wherever the label is background
    return logits.to(dtype).contiguous(), labels.to(torch.uint8).contiguous()


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


def desc(t, c):
    n, h, w, ld = t.shape
    return L.IsaTensor(t.data_ptr(), n, h, w, c, ld, L.dtype_code(t.dtype), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--classes", default="2,8,32")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sem_score_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sem_score.py needs the GPU"
    lib, st, B = L.lib(), L.stream_ptr(), opt.batch
    lines = ["sem score bench: %s, B=%d; host: best of %d calls (host clock), device: events over %d calls after %d warm-up"
             % (torch.cuda.get_device_name(0), B, opt.host_calls, opt.calls, opt.warmup)]
    for size in [int(v) for v in opt.sizes.split(",")]:
        Lp = size * size
        for K in [int(v) for v in opt.classes.split(",")]:
            for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
                for dist in ("background", "uniform"):
                    logits, labels = make_inputs(B, size, K, dtype, dist, seed=size + K)
                    x = desc(logits, K)
                    conf = torch.empty((B, K, K), dtype=torch.int64, device="cuda")
                    oob = torch.empty((B,), dtype=torch.int32, device="cuda")
                    cmap = torch.empty((B, Lp), dtype=torch.uint8, device="cuda")
                    amap = torch.empty((B, size, size, 8), dtype=dtype, device="cuda")
                    y = desc(amap, 1)
                    hist = torch.empty((B, K, K), dtype=torch.int32, device="cuda")
                    hoob = torch.empty((B,), dtype=torch.int32, device="cuda")

                    def fused(with_map=True):
                        L.check(lib.isa_sem_confusion(C.byref(x), L.ptr(labels), K, L.ptr(conf), L.ptr(oob),
                                                      L.ptr(cmap) if with_map else None, st), "isa_sem_confusion")

                    def unfused():
                        L.check(lib.isa_chan_argmax(C.byref(x), C.byref(y), st), "isa_chan_argmax")
                        pred = amap[..., 0].to(torch.uint8)
                        L.check(lib.isa_label_pair_hist(L.ptr(labels), L.ptr(pred), B, Lp, K, K, L.ptr(hist), L.ptr(hoob),
                                                        L.HIST_AGGREGATE, st), "isa_label_pair_hist")
                        return pred

                    def host():
                        probs = torch.empty((B, K, size, size), dtype=torch.float32, device="cuda")
                        L.check(lib.isa_softmax_nchw(C.byref(x), L.ptr(probs), st), "isa_softmax_nchw")
                        p, lab = probs.cpu().numpy(), labels.cpu().numpy().reshape(B, -1).astype(np.int64)
                        pred = p.argmax(1).reshape(B, -1)
                        return np.stack([np.bincount(lab[i] * K + pred[i], minlength=K * K).reshape(K, K) for i in range(B)])

                    fused()
                    pred_b = unfused()
                    torch.cuda.synchronize()
                    assert torch.equal(conf, hist.long()) and int(oob.sum()) == 0 and int(hoob.sum()) == 0
                    assert torch.equal(cmap.view(-1), pred_b.reshape(-1))
                    share00 = float(conf[:, 0, 0].sum()) / (B * Lp)
                    tag = "%4d x %-4d K=%-2d %s %-10s" % (size, size, K, dname, dist)
                    if dist == "background":
                        assert share00 >= 0.95, share00
                        ts = []
                        for _ in range(opt.host_calls):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            h = host()
                            ts.append((time.perf_counter() - t0) * 1e3)
                        # softmax rounding can merge the two largest probabilities of a pixel whose logits differ: the host
                        # arg-max may then name another class there; report the count instead of asserting equality
                        moved = int(np.abs(h - conf.cpu().numpy()).sum()) // 2
                        lines.append("%s (a) host %10.2f ms  (%d MB softmax download; %d of %d pixels counted elsewhere)"
                                     % (tag, min(ts), B * K * Lp * 4 >> 20, moved, B * Lp))
                    t_b = event_us(unfused, opt.calls, opt.warmup)
                    t_c = event_us(fused, opt.calls, opt.warmup)
                    t_alone = event_us(lambda: fused(False), opt.calls, opt.warmup)
                    nbytes = logits.numel() * logits.element_size() + labels.numel()
                    lines.append("%s (b) unfused %8.1f us   (c) isa_sem_confusion %8.1f us   (b) / (c) %5.2f   (0,0) share %.3f"
                                 % (tag, t_b, t_c, t_b / t_c, share00))
                    lines.append("%s isa_sem_confusion alone, counters only: %8.1f us per call (2 memsets + kernel) = %6.0f GB/s "
                                 "of the %d bytes it must read" % (tag, t_alone, nbytes / t_alone / 1e3, nbytes))
                    del logits, labels, amap, cmap
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
