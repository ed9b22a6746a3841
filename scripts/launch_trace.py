#!/usr/bin/env python3
"""Ordered launch trace of one instrumented eager step at 64 x 64, B = 2, after two warm-up steps: one line
`entry_point algorithmic_bytes` per launch, in host issue order.  Two builds that print the same trace issue the same
launches (and replay the same graph); environment flags (ISA_STREAMS, ISA_INLINE_FIN, ISA_FUSE_* ...) apply as usual.
usage: python scripts/launch_trace.py [train|eval|eval_head] [bf16|f32] > trace.txt    (diff two of them)
       python scripts/launch_trace.py --counts trace.txt ...                            (launches per entry point)"""
import collections, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 2 and sys.argv[1] == "--counts":
    for path in sys.argv[2:]:
        n = collections.Counter(line.split()[0] for line in open(path) if line.strip())
        print("\n== %s: %d launches" % (os.path.basename(path), sum(n.values())))
        for kv in sorted(n.items()):
            print("  %-34s %5d" % kv)
    sys.exit(0)

import torch
import isa_amd  # noqa
from isa_amd.reseg import ReSeg
from isa_amd.trainer import Trainer
from isa_amd.data import synth_batch

mode = sys.argv[1] if len(sys.argv) > 1 else "train"
dtype = torch.float32 if (len(sys.argv) > 2 and sys.argv[2] == "f32") else torch.bfloat16
torch.manual_seed(0)
m = ReSeg(2, mode != "eval", dtype=dtype).cuda()
x, sem, ins, n = synth_batch(2, 64, 64, seed=0)
x, sem, ins = x.cuda(), sem.cuda(), ins.cuda()
if mode == "train":
    tr = Trainer(m.train())
    step = lambda: tr.forward_backward(x, sem, ins, n)
elif mode == "eval":
    m.eval()
    step = lambda: m(False, x)
else:
    m.eval()
    step = lambda: m(False, x, sem, ins, n)
E = m.engine
with torch.set_grad_enabled(mode == "train"):
    for i in range(3):
        E.profile = i == 2
        step()
torch.cuda.synchronize()
for name, s, e, nbytes in E.prof_events:
    print(name, int(nbytes))
