#!/usr/bin/env python3
"""Time of ground-truth-free instance inference (ReSeg.segment) against the ground-truth eval forward.

Both sides run the same decoder passes on the same points: synth_batch with `--objects` objects in every image, the GT
foreground as sem_map, and the points of the GT path injected into segment().
  baseline: forward(False, x, sem, ins, N) in eval mode - per iteration the instance softmax, the arg-max, the pyramid
            targets, a full decoder pass (cross branches included) and the loss sums;
  segment : the cross branches once per call, per iteration the level chain and isa_seg_claim.
Calls alternate (baseline, segment, baseline, ...), each ends in a device synchronise and is timed with the host
clock; the median of `--calls` calls after `--warmup` is reported, with the quartiles.  "per iteration after the
first" is (time with T points - time with 1 point) / (T - 1) from a second pair of alternating series.  Entry-point
calls and the time of isa_seg_claim come from one extra call with the engine's event profiler on (not a timed call).
isa_seg_claim alone is also timed on a map that is all foreground and never claimed (it then reads every byte it can).
Needs a GPU; there is no fallback.  Appends its lines to --out."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import isa_amd  # noqa: F401,E402
import reseg_ref as R  # noqa: E402
from isa_amd import lib as L  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, calls, warmup):
    """Median and quartiles (ms) of each function, the functions called in turn."""
    for _ in range(warmup):
        for f in fns:
            timed(f)
    ts = [[] for _ in fns]
    for _ in range(calls):
        for i, f in enumerate(fns):
            ts[i].append(timed(f))
    out = []
    for t in ts:
        q = statistics.quantiles(t, n=4)
        out.append((statistics.median(t), q[0], q[2]))
    return out


def profiled_calls(model, fn):
    """{entry point: (calls, ms)} of one call of fn under the engine's event profiler."""
    E = model.engine
    E.profile, E.prof_events = True, []
    fn()
    torch.cuda.synchronize()
    out = {}
    for name, s, e, _ in E.prof_events:
        c, ms = out.get(name, (0, 0.0))
        out[name] = (c + 1, ms + s.elapsed_time(e))
    E.profile, E.prof_events = False, []
    return out


def claim_alone(n, hw, dtype, ld, reps=50):
    """us per isa_seg_claim call on an all-foreground map whose pixels are never claimed (l1 < l0, point aside)."""
    lib = L.lib()
    Lp = hw * hw
    sem = torch.ones(n, Lp, device="cuda")
    merge = torch.rand(n, Lp, device="cuda")
    pred = torch.zeros(n, hw, hw, ld, dtype=dtype, device="cuda")
    pred[..., 0] = 1.0
    desc = L.IsaTensor(pred.data_ptr(), n, hw, hw, 2, ld, L.dtype_code(dtype), 1)
    labels = torch.empty(n, Lp, dtype=torch.uint8, device="cuda")
    ints = torch.zeros(3 * n + 4, dtype=torch.int32, device="cuda")
    count, active, s_t, anyw = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:]
    part = torch.empty(n * 128, device="cuda")
    st = L.stream_ptr()
    L.check(lib.isa_seg_begin(L.ptr(sem), L.ptr(merge), n, Lp, L.ptr(labels), L.ptr(count), L.ptr(s_t), L.ptr(active),
                              L.ptr(anyw), L.ptr(part), st), "isa_seg_begin")

    def call():
        L.check(lib.isa_seg_claim(desc, L.ptr(sem), L.ptr(merge), L.ptr(s_t), L.ptr(labels), L.ptr(count), L.ptr(active),
                                  L.ptr(s_t), L.ptr(anyw), L.ptr(part), st), "isa_seg_claim")
    for _ in range(5):
        call()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segment.py needs the GPU"
    assert opt.calls >= 20, "median of at least 20 timed calls"
    lines = ["segment bench: %s, %dx%d, B=%d, %d objects per image, median [q1, q3] of %d alternating calls after %d warm-up"
             % (torch.cuda.get_device_name(0), opt.size, opt.size, opt.batch, opt.objects, opt.calls, opt.warmup)]
    B, size = opt.batch, opt.size
    x, sem, ins, n = R.synth_batch(B, size, size, seed=0, kmin=opt.objects, kmax=opt.objects)
    T = int(n.min())
    assert T == opt.objects, "synth_batch placed %d objects in some image, not %d" % (T, opt.objects)
    sel = [list(range(int(k))) for k in n.view(-1)]
    xd, semd, insd = x.cuda(), sem.cuda(), ins.cuda()
    fg = semd[:, 1].float().reshape(B, -1).contiguous()
    for name in opt.dtypes.split(","):
        dtype = dict(bf16=torch.bfloat16, fp32=torch.float32)[name]
        m = ReSeg(2, True, dtype=dtype)
        m.load_state_dict(R.synth_state_dict())
        m.eval()
        m.head.drop_rate = 0.0
        with torch.no_grad():
            m(False, xd, semd, insd, n, selected_idx=sel)
            points = [r["s_t"].clone() for r in m.last_record["iters"]]
            assert len(points) == T
            base = lambda: m(False, xd, semd, insd, n, selected_idx=sel)
            seg = lambda: m.segment(xd, sem_map=fg, injected_s_t=points)
            seg1 = lambda: m.segment(xd, sem_map=fg, injected_s_t=points[:1])
            n1 = torch.ones_like(n)
            base1 = lambda: m(False, xd, semd, insd, n1, selected_idx=sel)
            free = lambda: m.segment(xd, max_objects=T, sem_map=fg)        # own points, stop test read every iteration
            (tb, tb1, tb3), (ts, ts1, ts3) = alternate([base, seg], opt.calls, opt.warmup)
            (tbo, _, _), (tso, _, _), (tf, tf1, tf3) = alternate([base1, seg1, free], opt.calls, opt.warmup)
            free()
            free_passes = m.head.seg_passes
            pc8, pc1 = profiled_calls(m, seg), profiled_calls(m, seg1)
            pb8, pb1 = profiled_calls(m, base), profiled_calls(m, base1)
        calls = lambda pc: sum(c for c, _ in pc.values())
        per_it = (calls(pc8) - calls(pc1)) / (T - 1)
        per_it_b = (calls(pb8) - calls(pb1)) / (T - 1)
        claim_n, claim_ms = pc8["isa_seg_claim"]
        lines += [
            "%s baseline forward(False, x, sem, ins, N=%d): %.2f ms [%.2f, %.2f]" % (name, T, tb, tb1, tb3),
            "%s segment, same %d points injected:          %.2f ms [%.2f, %.2f]   ratio segment / baseline %.3f"
            % (name, T, ts, ts1, ts3, ts / tb),
            "%s segment, own points + stop test:          %.2f ms [%.2f, %.2f]   (%d passes)" % (name, tf, tf1, tf3, free_passes),
            "%s per iteration after the first: segment %.2f ms, baseline %.2f ms (ratio %.3f); one iteration: segment %.2f ms, "
            "baseline %.2f ms" % (name, (ts - tso) / (T - 1), (tb - tbo) / (T - 1), (ts - tso) / max(tb - tbo, 1e-9), tso, tbo),
            "%s entry-point calls per iteration after the first: segment %.1f (isa_seg_claim = 2 kernel launches), baseline %.1f; "
            "whole call: segment %d, baseline %d" % (name, per_it, per_it_b, calls(pc8), calls(pb8)),
            "%s isa_seg_claim inside the run (events around both launches): %.1f us per call" % (name, claim_ms / claim_n * 1e3),
        ]
        Lp = size * size
        for ld in (8, 2):
            us = claim_alone(B, size, dtype, ld)
            esz = 4 if dtype == torch.float32 else 2
            alg = B * Lp * (4 + 4 + 1 + 2 * esz)                   # sem + merge + labels read + the two logits
            touched = B * Lp * (4 + 4 + 1 + max(ld * esz, 2 * esz))   # ld = 8: the whole pixel stride is fetched
            lines.append("%s isa_seg_claim alone, all %d x %d pixels remaining, pred ld=%d: %.1f us per call (2 launches) = "
                         "%.0f GB/s of the %d bytes it needs, %.0f GB/s of the %d bytes its loads touch"
                         % (name, B, Lp, ld, us, alg / us / 1e3, alg, touched / us / 1e3, touched))
        del m
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
