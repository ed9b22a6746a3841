#!/usr/bin/env python3
"""Ordered launch trace of one instrumented eager step at 64 x 64, B = 2, after two warm-up steps: one line
`entry_point algorithmic_bytes` per launch, in host issue order.  Two builds that print the same trace issue the same
launches (and replay the same graph); environment flags (ISA_STREAMS, ISA_INLINE_FIN, ISA_FUSE_* ...) apply as usual.
After the line `== streams` the same step in a second form: `stream entry_point` per launch (the engine's stream id at
call time) and `sync src dst` per stream edge (Engine.sync with src != dst), in host order - two builds that agree here
also put every launch on the same stream and order the streams by the same edges.
Modes: train (Trainer.forward_backward), train1 (the same with one object in the first image: one decoder iteration),
train_terms (train with the border-weighted CE and the discriminative loss on: Trainer(border_weight=10, disc_weight=1)),
train_eval (train() module called with training=False on a batch whose smallest image has four objects: four
iterations with batch statistics), eval_head (eval() module with ground truth), eval (no instance head).
usage: python scripts/launch_trace.py [train|train1|train_terms|train_eval|eval|eval_head] [bf16|f32] > trace.txt    (diff two of them)
       python scripts/launch_trace.py --counts trace.txt ...                            (launches per entry point)"""
import collections, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SECOND = "== streams"

if len(sys.argv) > 2 and sys.argv[1] == "--counts":
    for path in sys.argv[2:]:
        first = itertools.takewhile(lambda line: line.strip() != SECOND, open(path))
        n = collections.Counter(line.split()[0] for line in first if line.strip())
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
x, sem, ins, n = synth_batch(2, 64, 64, seed=2 if mode == "train_eval" else 0)
x, sem, ins = x.cuda(), sem.cuda(), ins.cuda()
if mode in ("train", "train1", "train_terms"):
    if mode == "train1":
        n[0] = 1
    tr = Trainer(m.train(), **(dict(border_weight=10.0, disc_weight=1.0) if mode == "train_terms" else {}))
    step = lambda: tr.forward_backward(x, sem, ins, n)
elif mode == "eval":
    m.eval()
    step = lambda: m(False, x)
else:
    m.train() if mode == "train_eval" else m.eval()
    step = lambda: m(False, x, sem, ins, n)
E = m.engine
placed = []                     # the second form, recorded while E.profile is set


class Recorder:
    """In front of E.lib: notes the engine's current stream with every entry point called through it."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            if E.profile:
                placed.append("%d %s" % (E.cur, name))
            return fn(*args)
        return call


def recorded_sync(src, dst, sync=E.sync):
    if E.profile and src != dst:
        placed.append("sync %d %d" % (src, dst))
    return sync(src, dst)


E.lib, E.sync = Recorder(E.lib), recorded_sync
with torch.set_grad_enabled(mode in ("train", "train1", "train_terms")):
    for i in range(3):
        E.profile = i == 2
        step()
torch.cuda.synchronize()
for name, s, e, nbytes in E.prof_events:
    print(name, int(nbytes))
print(SECOND)
print("\n".join(placed))
