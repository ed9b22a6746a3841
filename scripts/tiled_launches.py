#!/usr/bin/env python3
"""Which isa_conv_gemm launches of one eager training step (256x256, batch 16, bf16) take the LDS-tiled small-GEMM
kernel, by shape: a stand-in for Engine.lib reads the arguments of every call and applies the dispatch condition of
launch0 in csrc/conv_gemm.hip (bf16, 1x1 plain, cin == kp, 128 <= kp <= 2048, kp % 64 == 0, N >= 64, N % 16 == 0, at most
65 536 pixels per statistic group; 128-wide tiles from 512 workgroups on).
usage: python scripts/tiled_launches.py"""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ISA_STREAMS", "1")
import torch
import isa_amd  # noqa
from isa_amd import lib as L
from isa_amd.reseg import ReSeg
from isa_amd.trainer import Trainer
from isa_amd.data import synth_batch


class Launches:
    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "isa_conv_gemm":
            return fn

        def call(x, pro, w, kp, bias, y, in_mode, out_mode, stats, acc, stream):
            xt, yt = x._obj, y._obj
            p = pro._obj if pro is not None else None
            has_pro = p is not None and bool(p.scale or p.shift or p.bscale or p.act != L.ACT_NONE)
            G = xt.groups if (xt.groups > 1 and (stats is not None or (p is not None and (p.scale or p.shift)))) else 1
            self._log.append((xt.n * xt.h * xt.w // G, G, xt.c, kp, yt.c, xt.dtype, in_mode, out_mode, has_pro,
                              p is not None and bool(p.bscale), p is not None and bool(p.fin), stats is not None, int(acc)))
            return fn(x, pro, w, kp, bias, y, in_mode, out_mode, stats, acc, stream)
        return call


torch.manual_seed(0)
m = ReSeg(2, True, dtype=torch.bfloat16).cuda().train()
tr = Trainer(m)
x, sem, ins, n = synth_batch(16, 256, 256, seed=0)
x, sem, ins = x.cuda(), sem.cuda(), ins.cuda()
for _ in range(2):
    tr.forward_backward(x, sem, ins, n)
torch.cuda.synchronize()
log = []
E = m.engine
E.lib = Launches(E.lib, log)
tr.forward_backward(x, sem, ins, n)
torch.cuda.synchronize()
bf16 = L.dtype_code(torch.bfloat16)
rows = collections.Counter()
other = 0
for M, G, cin, kp, N, dt, im, om, has_pro, bs, fin, stats, acc in log:
    if dt == bf16 and im == L.IN_1X1 and om == L.OUT_PLAIN and cin == kp and 128 <= kp <= 2048 and kp % 64 == 0 and N >= 64 \
            and N % 16 == 0 and M <= 65536:
        wide = N >= 128 and ((M + 127) // 128) * ((N + 127) // 128) * G >= 512
        rows[(M, G, kp, N, 2 if wide else 1, "pro" if has_pro else "-", "bs" if bs else "-", "fin" if fin else "-",
              "stats" if stats else "-", "acc" if acc else "-")] += 1
    else:
        other += 1
print("isa_conv_gemm: %d launches, %d through conv_gemm_tiled_kernel, %d through the other kernels" % (len(log), sum(rows.values()), other))
print("%8s %2s %5s %5s %3s %4s %3s %4s %6s %4s %9s %8s" % ("pixels", "G", "K", "N", "WN", "pro", "bs", "fin", "stats", "acc", "MB/launch", "launches"))
for k, c in sorted(rows.items(), key=lambda kv: (-kv[0][0] * kv[0][1] * (kv[0][2] + kv[0][3]), kv[0])):
    M, G, kp, N = k[:4]
    print("%8d %2d %5d %5d %3d %4s %3s %4s %6s %4s %9.2f %8d" % (k + (M * G * (kp + N) * 2 / 1e6, c)))
