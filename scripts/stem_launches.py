#!/usr/bin/env python3
"""Backward launches of the instance stems (InstanceHead.stems) in instrumented eager training steps: entry point,
algorithmic MB, us and GB/s per launch in tape order of the backward pass, their sum, and the whole step for scale.
The step is scripts/step_shapes.py's (256x256, 16 images, bf16, one stream, Engine.profile).  stems() is wrapped: the tape
entries it records are replaced by closures that note which profiled launches each of them issues when the backward
pass runs it.
usage: python scripts/stem_launches.py [tree root]      (another checkout of the project, e.g. the parent commit's, with
its own library; default: this one.  ISA_FUSE_BIAS=0 selects the separate kernels.)"""
import os, sys
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ISA_STREAMS", "1")
import torch
import isa_amd  # noqa
from isa_amd.reseg import ReSeg
from isa_amd.trainer import Trainer
from isa_amd.data import synth_batch
from isa_amd.instance_head import InstanceHead

torch.manual_seed(0)
m = ReSeg(2, True, dtype=torch.bfloat16).cuda().train()
tr = Trainer(m)
x, sem, ins, n = synth_batch(16, 256, 256, seed=0)
x, sem, ins = x.cuda(), sem.cuda(), ins.cuda()
E = m.engine
spans = []
orig = InstanceHead.stems


def stems(self, x_dec):
    tape = self.E.tape
    a = len(tape)
    out = orig(self, x_dec)
    for i in range(a, len(tape)):
        fn, sid = tape[i]
        if fn is None:
            continue

        def wrapped(fn=fn, i=i):
            s = len(E.prof_events)
            fn()
            spans.append((i, s, len(E.prof_events)))
        # keep identity checks of the engine (bn.bwd_fn is tape.last_fn()) out of harm's way: they ran during recording
        list.__setitem__(tape, i, (wrapped, sid))
    return out


InstanceHead.stems = stems
for _ in range(2):
    tr.forward_backward(x, sem, ins, n)
torch.cuda.synchronize()
for rep in range(3):
    spans.clear()
    E.prof_events = []
    E.profile = True
    tr.forward_backward(x, sem, ins, n)
    torch.cuda.synchronize()
    E.profile = False
    ev = E.prof_events
    tot, cnt = 0.0, 0
    print("--- instrumented step %d: stems backward launches (tape order)" % rep)
    print("%-34s %10s %9s %8s" % ("entry point", "MB", "us", "GB/s"))
    for i, s, e in spans:
        for name, a, b, nb in ev[s:e]:
            t = a.elapsed_time(b) * 1e3
            tot += t; cnt += 1
            print("%-34s %10.2f %9.1f %8.0f" % (name, nb / 1e6, t, nb / 1e3 / t if t else 0))
    print("stems backward: %d launches, %.1f us" % (cnt, tot))
    allt = sum(a.elapsed_time(b) for _, a, b, _ in ev)
    print("whole instrumented step: %d launches, %.2f ms" % (len(ev), allt))
